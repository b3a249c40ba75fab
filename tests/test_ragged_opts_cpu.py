"""No GPU: the device-free half of the ragged option calls (Sampler.begin_ragged's keywords, mmdm_begin_ragged_opts) -- how lists and packed tensors
become the packed buffers the library takes, the default noise rows, every shape error -- and the generator identity the GPU tests rest on."""
import numpy as np
import pytest
import torch

from test_sampler_opts_cpu import step_normal_f64

LENS = (5, 1, 3)
SUM = sum(LENS)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_lists_and_packed_tensors_give_the_same_buffers():
    from mixermdm_amd.sampler import pack_ragged_options
    noise = [rnd(10 + b, 4, t, 524) for b, t in enumerate(LENS)]
    xs = [rnd(20 + b, t + b, 524) for b, t in enumerate(LENS)]                  # items 1, 2 hold more frames than the call: cut to T_i
    init = [rnd(30 + b, t, 524) for b, t in enumerate(LENS)]
    a = pack_ragged_options(LENS, noise=noise, x_start=xs, init_image=init, skip_timesteps=1)
    assert a["noise"].shape == (4, SUM, 524) and a["x_start"].shape == (SUM, 524) and a["init_image"].shape == (SUM, 524)
    o = 0
    for b, t in enumerate(LENS):                                                # within a slot the items lie back to back, as x_T does
        assert torch.equal(a["noise"][:, o:o + t], noise[b])
        assert torch.equal(a["x_start"][o:o + t], xs[b][:t])
        assert torch.equal(a["init_image"][o:o + t], init[b])
        o += t
    p = pack_ragged_options(list(LENS), noise=a["noise"], x_start=a["x_start"], init_image=a["init_image"], skip_timesteps=1)
    for k in ("noise", "x_start", "init_image"):
        assert torch.equal(p[k], a[k]) and p[k].is_contiguous() and p[k].dtype == torch.float32
    assert a["seeds"] is None and a["noise_rows"] is None and a["skip_timesteps"] == 1
    # float64 input is converted, nothing else is touched
    d = pack_ragged_options(LENS, init_image=[t.double() for t in init])
    assert d["init_image"].dtype == torch.float32 and torch.equal(d["init_image"], a["init_image"])
    assert d["noise"] is None and d["x_start"] is None and d["skip_timesteps"] == 0


def test_default_noise_rows_for_one_seed_and_for_a_sequence():
    from mixermdm_amd.sampler import pack_ragged_options
    one = pack_ragged_options(LENS, seeds=7)
    assert one["seeds"] == [7, 7, 7] and one["noise_rows"] == [0, 1, 2]         # the batch is ONE call: item b is its batch row b
    each = pack_ragged_options(LENS, seeds=[7, 8, 9])
    assert each["seeds"] == [7, 8, 9] and each["noise_rows"] == [0, 0, 0]       # every item its own B = 1 call
    rows = pack_ragged_options(LENS, seeds=[7, 7, 9], noise_rows=[0, 1, 0])     # explicit rows override (sample_many: calls of more than one motion)
    assert rows["seeds"] == [7, 7, 9] and rows["noise_rows"] == [0, 1, 0]
    assert pack_ragged_options(LENS, seeds=np.int64(7), noise_rows=(2, 2, 2))["noise_rows"] == [2, 2, 2]
    assert pack_ragged_options(LENS, seeds=[-1, 1 << 64, 5])["seeds"] == [(1 << 64) - 1, 0, 5]      # 64-bit keys


@pytest.mark.parametrize("kw", [
    dict(noise=torch.zeros(4, SUM, 524), seeds=3),                              # both noise forms
    dict(noise_rows=[0, 0, 0]),                                                 # rows without seeds
    dict(noise=torch.zeros(4, SUM + 1, 524)),
    dict(noise=torch.zeros(SUM, 524)),
    dict(noise=torch.zeros(4, SUM, 262)),
    dict(noise=[torch.zeros(4, 5, 524), torch.zeros(4, 1, 524)]),               # two items for three
    dict(noise=[torch.zeros(4, 5, 524), torch.zeros(3, 1, 524), torch.zeros(4, 3, 524)]),   # another n
    dict(noise=[torch.zeros(4, 5, 524), torch.zeros(4, 2, 524), torch.zeros(4, 3, 524)]),   # another T_i
    dict(seeds=[1, 2]),
    dict(seeds=[1, 2, 3], noise_rows=[0, 0]),
    dict(seeds=[1, 2, 3], noise_rows=[0, -1, 0]),
    dict(x_start=torch.zeros(SUM - 1, 524)),
    dict(x_start=torch.zeros(1, SUM, 524)),
    dict(x_start=[torch.zeros(5, 524), torch.zeros(1, 524), torch.zeros(2, 524)]),          # fewer frames than the item
    dict(x_start=[torch.zeros(5, 524), torch.zeros(1, 524)]),
    dict(x_start=[torch.zeros(5, 524), torch.zeros(1, 524), torch.zeros(3, 262)]),
    dict(init_image=torch.zeros(SUM, 523)),
    dict(init_image=[torch.zeros(5, 524), torch.zeros(1, 524), torch.zeros(4, 524)]),       # init_image is T_i frames exactly
    dict(init_image=[torch.zeros(5, 524), torch.zeros(1, 524)]),
])
def test_every_shape_error_raises(kw):
    from mixermdm_amd.sampler import pack_ragged_options
    with pytest.raises(ValueError, match="ragged options"):
        pack_ragged_options(LENS, **kw)


def test_lens_errors_raise():
    from mixermdm_amd.sampler import pack_ragged_options
    for lens in ((), (3, 0)):
        with pytest.raises(ValueError, match="ragged options"):
            pack_ragged_options(lens, seeds=1)


def test_options_struct_mirrors_the_header():
    """mmdm_begin_ragged_options as ctypes lays it out == the C struct's natural layout (field order of include/mmdm.h)."""
    import ctypes as C
    import os
    import re
    from mixermdm_amd._lib import BeginRaggedOptions, SYMBOLS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmdm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mmdm_begin_ragged_options;", hdr).group(1)
    names = [re.search(r"(\w+)(\[\d+\])?;", ln).group(1) for ln in body.strip().split("\n")]
    assert names == [f[0] for f in BeginRaggedOptions._fields_]
    assert "mmdm_begin_ragged_opts" in SYMBOLS and len(SYMBOLS["mmdm_begin_ragged_opts"][1]) == 7
    assert C.sizeof(BeginRaggedOptions) == 64 and BeginRaggedOptions.init_coef.offset == 52


def test_generator_identity_of_a_ragged_item():
    """The generator's counter is (t * 524 + column, b, loop position, 0): it holds neither B nor T.  So item b of a call of B items seeded `seed`
    draws what row `b` of ANY call with that seed draws (one seed: noise row b), and an item with its own seed draws row 0 of a B = 1 call
    (a sequence of seeds: noise row 0) -- whatever the lengths of the items beside it."""
    seed, k = 0x1234_5678_9ABC_DEF1, 2
    whole = step_normal_f64(seed, k, 3, 7)                                      # the uniform B = 3, T = 7 call
    for b, t in enumerate((7, 2, 5)):                                           # (seed, row b) at the item's own length
        assert np.array_equal(step_normal_f64(seed, k, b + 1, t)[b], whole[b, :t])
    alone = [step_normal_f64(seed + b, k, 1, t)[0] for b, t in enumerate((7, 2, 5))]          # (seed_b, row 0)
    for b, t in enumerate((7, 2, 5)):
        assert np.array_equal(alone[b], step_normal_f64(seed + b, k, 4, 9)[0, :t])
        assert np.array_equal(alone[b], whole[b, :t]) == (b == 0)               # (seed + 0, row 0) is row 0 of the whole; another key or row is not
    assert not np.array_equal(whole[0], whole[1])
