"""GPU: ragged batches (mmdm_begin_ragged) with MDMDenoiser as MODEL1 (model1_kind = 1; src/models/mixermdm.py:32-40, src/models/mdm.py:234-298).

The MDM encoder runs on TOKEN rows -- every item's conditioning token in front of its frames -- so a ragged call has two row spaces (frame groups and
token groups, each with its own stride and maps) and the plain-softmax attention (MMDM_ATTN_NO_ZERO_KEY) walks ragged token sequences.  Everything here
is held by bit-identity with the stand-alone calls, which tests/test_gpu_extensions.py and the mdm.npz goldens hold to the reference."""
import ctypes as C
import os
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

# the other stacks as in tests/test_gpu_ragged.py; denoiser 1 = MDM, D1 = 128, H1 = 2 (head size 64), two layers
DIMS = dict(d_latent=128, d_ff=256, d_layers=2, m_latent=128, m_ff=256, m_layers=2)
LENS = (40, 17, 64, 1, 33)
NO_ZERO_KEY, CAUSAL = 1, 2


def small(max_batch=8, max_frames=64, single_only=False, d1=(128, 256, 2, 2), d_heads=2):
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict, synthetic_stats
    D1, F1, L1, H1 = d1
    sd = synthetic_state_dict(seed=7, std=0.05, bias_std=0.02, mixing_mode=4, model1="MDM", single_only=bool(single_only), d1_latent=D1, d1_ff=F1, d1_layers=L1, **DIMS)
    s = Sampler(d_heads=d_heads, m_heads=2, max_batch=max_batch, max_frames=max_frames, mixing_mode=4, single_only=single_only, model1_kind=1,
                d1_latent=D1, d1_ff=F1, d1_layers=L1, d1_heads=H1, **DIMS)
    s.load_state_dict(sd)
    if not single_only:
        st = synthetic_stats()
        s.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
    s.prepare()
    s.set_schedule("ddim20")
    return s


def inputs(lens, width=524, cw=6 * 768 + 2 * 128, seed=0):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(len(lens), cw, generator=g)
    xs = [torch.randn(t, width, generator=g) for t in lens]
    return cond, xs


def alone(s, cond, xs):
    return [s.sample(cond[b:b + 1], x[None])[0] for b, x in enumerate(xs)]


def check_items(s, cond, xs, lens, ref, **kw):
    items = s.sample_ragged(cond, xs, lens, **kw)
    for b, (it, r) in enumerate(zip(items, ref)):
        assert it.shape == r.shape and torch.isfinite(it).all(), (b, lens[b])
        assert torch.equal(it, r), (b, lens[b], (it - r).abs().max().item())


# ---------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [64, 128])
def test_ragged_plain_softmax_attention_is_the_uniform_kernel_per_sequence(dh):
    """mmdm_attention_ragged_opts_f32 with MMDM_ATTN_NO_ZERO_KEY: the empty initial state (m = -inf, l = 0) through the ragged walk -- sequences of one
    key, a partial last chunk (5, 70, 129, 300), query tiles and waves past a sequence's end (1, 2, 5, 16 in a grid sized for 300)."""
    from mixermdm_amd._lib import load_library, check, MMDMError
    lib = load_library()
    H, D = 2, 2 * dh
    lens = [70, 5, 64, 129, 16, 2, 1, 300]
    nseq, total = len(lens), sum(lens)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    g = torch.Generator().manual_seed(dh)
    qkv = torch.randn(total + 7, 3 * D, generator=g).cuda()         # rows behind the last sequence exist and hold data
    out = torch.full((total, D), float("nan"), device="cuda")
    d_off, d_len = torch.from_numpy(off).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + 4 * o)
    check(lib.mmdm_attention_ragged_opts_f32(p(qkv), 3 * D, p(qkv, D), 3 * D, p(qkv, 2 * D), 3 * D, p(out), D, NO_ZERO_KEY, nseq, p(d_off), p(d_len),
                                             max(lens), total, H, dh, 0, None))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    for s, (o, t) in enumerate(zip(off, lens)):
        ref = torch.empty(t, D, device="cuda")
        q = qkv[o:o + t].contiguous()
        check(lib.mmdm_attention_opts(p(q), 3 * D, p(q, D), 3 * D, p(q, 2 * D), 3 * D, p(ref), D, 0, NO_ZERO_KEY, 1, t, t, H, dh, 0, None))
        torch.cuda.synchronize()
        assert torch.equal(out[o:o + t], ref), (s, t)
    # the ops wrapper is the same launch
    from mixermdm_amd import ops
    out2 = ops.attention_ragged(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], H, d_off, d_len, max(lens), zero_key=False)
    torch.cuda.synchronize()
    assert torch.equal(out2[:total], out)
    # a causal mask on a ragged launch stays refused
    with pytest.raises(MMDMError, match="ragged"):
        check(lib.mmdm_attention_ragged_opts_f32(p(qkv), 3 * D, p(qkv, D), 3 * D, p(qkv, 2 * D), 3 * D, p(out), D, NO_ZERO_KEY | CAUSAL, nseq, p(d_off), p(d_len),
                                                 max(lens), total, H, dh, 0, None))


# ---------------------------------------------------------------------------------------------------
# the two-chain sampler
# ---------------------------------------------------------------------------------------------------
def test_ragged_mdm_batch_items_equal_their_stand_alone_calls():
    s = small()
    cond, xs = inputs(LENS, seed=4)
    names = ("influence_i1", "influence_i2", "out_influenced")
    ref, ref_hist = [], []
    for b, x in enumerate(xs):
        out, hist = s.sample(cond[b:b + 1], x[None], history=names, history_every=5)
        ref.append(out[0])
        ref_hist.append(hist)
    items, hist, ev = s.sample_ragged_async(cond, xs, LENS, history=names, history_every=5)       # (graph replay)
    ev.synchronize()
    assert s.rows % 128 == 0 and s.rows >= sum(LENS)
    for b, ((o, t), it) in enumerate(zip(s.item_slices(), items)):
        assert torch.equal(it, ref[b]), (b, (it - ref[b]).abs().max().item())
        for k, v in hist.items():            # [slots, 2, rows, C] vs the stand-alone [slots, 2B = 2, T, C]
            assert torch.equal(v[:, :, o:o + t], ref_hist[b][k]), (k, b)
    # eager == graph, and a batch in another order gives the same motions
    check_items(s, cond, xs, LENS, ref, use_graph=False)
    perm = [3, 0, 4, 2, 1]
    check_items(s, cond[perm], [xs[i] for i in perm], [LENS[i] for i in perm], [ref[i] for i in perm], use_graph=False)
    s.close()


def test_ragged_mdm_at_the_token_tile_edges():
    """len + 1 = 2, 16, 17, 18, 32, 33, 64, 65: the 16-key stage, the 16-query wave and the 64-query workgroup edges of the TOKEN sequences."""
    lens = (1, 15, 16, 17, 31, 32, 63, 64)
    s = small(max_batch=8, max_frames=64)
    cond, xs = inputs(lens, seed=11)
    check_items(s, cond, xs, lens, alone(s, cond, xs))
    s.close()


def test_ragged_mdm_frame_and_token_strides_are_independent():
    """(60, 60, 6): 126 frames -> 128 frame rows, 129 tokens -> 256 token rows (default bucket 128)."""
    lens = (60, 60, 6)
    s = small()
    cond, xs = inputs(lens, seed=12)
    ref = alone(s, cond, xs)
    check_items(s, cond, xs, lens, ref)
    assert s.rows == 128
    s.close()


def test_ragged_mdm_strides_clipped_to_the_workspace():
    """max_batch x max_frames = 128 frame rows and 130 token rows are all there is: both strides are clipped to capacity, not rounded up to 256."""
    lens = (64, 64)
    s = small(max_batch=2, max_frames=64)
    cond, xs = inputs(lens, seed=13)
    check_items(s, cond, xs, lens, alone(s, cond, xs))
    assert s.rows == 128
    s.close()


def test_ragged_mdm_graphs_are_keyed_by_the_token_geometry_too():
    """Same B and the same frame stride (128) throughout.  (60, 60, 6): token stride 256.  (60, 60, 5) and (64, 60, 1): token stride 128 and one frame
    tile each (64 frames), but 61 tokens are one query tile and 65 tokens are two."""
    s = small()
    seq = [(60, 60, 6), (60, 60, 5), (64, 60, 1), (60, 60, 6)]
    for i, lens in enumerate(seq):
        cond, xs = inputs(lens, seed=20 + sum(lens))
        ref = s.sample_ragged(cond, xs, lens, use_graph=False)
        got = s.sample_ragged(cond, xs, lens, use_graph=True)
        assert s.rows == 128
        for x, y in zip(ref, got):
            assert torch.equal(x, y), (i, lens)
        cap, rep, cached = s.graph_stats()
        assert (cap, cached) == (min(i + 1, 3), min(i + 1, 3)) and rep == 20 * (i + 1), (i, cap, rep, cached)
    s.close()


# ---------------------------------------------------------------------------------------------------
# the single-person sampler
# ---------------------------------------------------------------------------------------------------
def test_ragged_single_person_mdm_sampler():
    s = small(single_only=1)
    cond, xs = inputs(LENS, width=262, cw=128, seed=5)
    check_items(s, cond, xs, LENS, alone(s, cond, xs))
    check_items(s, cond, xs, LENS, alone(s, cond, xs), use_graph=False)
    s.close()


def test_ragged_mdm_larger_denoiser_state_after_two_steps():
    """D1 = 256, four heads, four layers, items up to 196 frames (four query tiles of tokens): x and pred_xstart after two steps, bitwise."""
    lens = (196, 60, 133, 1)
    s = small(max_batch=4, max_frames=196, single_only=1, d1=(256, 512, 4, 4))
    cond, xs = inputs(lens, width=262, cw=256, seed=6)
    ref = []
    for b, x in enumerate(xs):
        s.begin(cond[b:b + 1], x[None])
        s.run(2)
        ref.append({k: v[0].clone() for k, v in s.state().items() if v is not None})
    s.begin_ragged(cond, xs, lens)
    s.run(2)
    st = s.state()
    for b, (o, t) in enumerate(s.item_slices()):
        for k in ("x", "pred_xstart"):
            assert torch.isfinite(st[k][o:o + t]).all()
            assert torch.equal(st[k][o:o + t], ref[b][k]), (k, b, t)
    s.close()


# ---------------------------------------------------------------------------------------------------
# the facade and the evaluation harness
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import MixerMDM
    root = tmp_path_factory.mktemp("cfg")
    sub = dict(NUM_LAYERS=2, NUM_HEADS=2, DROPOUT=0.1, INPUT_DIM=262, LATENT_DIM=128, FF_SIZE=256)
    for name, nm in [("mdm.yaml", "MDM"), ("in2IN.yaml", "in2IN")]:
        yaml.safe_dump(dict(NAME=nm, **sub), open(root / name, "w"))
    cfg = CfgNode(dict(NAME="MixerMDM", GENERATOR=dict(sub), DISCRIMINATOR=dict(sub), ACTIVATION="gelu", DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine",
                       SAMPLER="uniform", MOTION_REP="global", CFG_WEIGHT=3.5, MIXING_MODE=4, FORCE_INFLUENCE_VAL="None", MODEL1="mdm.yaml", MODEL2="in2IN.yaml"))
    m = MixerMDM(cfg, num_frames=64, sampling_strategy="ddim20", config_root=str(root))
    m.init_synthetic(seed=0, std=0.05, bias_std=0.02)
    m = m.to("cuda:0").eval()
    assert m.model1_kind == 1 and m.mixing.denoiser1.text_dim == 128
    return m


CW = 6 * 768 + 2 * 128


def test_facade_sample_many_ragged_equals_the_per_item_loop_with_mdm(model):
    lens, reps = (40, 17, 64, 33), (1, 1, 2, 1)
    batches = []
    for i, (t, r) in enumerate(zip(lens, reps)):
        g = torch.Generator().manual_seed(i)
        batches.append({"cond": torch.randn(r, CW, generator=g).cuda(), "x_T": torch.randn(r, t, 524, generator=g).cuda(), "motion_lens": torch.tensor([t]), "text": ["x"] * r})
    ref = [model.forward_test(dict(b)) for b in batches]
    ref = [{k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in r.items()} for r in ref]
    got = model.sample_many([dict(b) for b in batches], batching="ragged")
    for r, g, t, nb in zip(ref, got, lens, reps):
        assert g["output"].shape == (nb, t, 524) and torch.equal(g["output"], r["output"]), t
        for k in ("influence_i1", "influence_i2"):
            assert len(g[k]) == len(r[k]) == 20
            for a, b in zip(g[k], r[k]):
                assert a.shape == b.shape and torch.equal(a, b), (k, t)


def test_evaluation_harness_ragged_equals_sequential_with_mdm(model):
    from mixermdm_amd.generation import generate_for_evaluation
    lens = (33, 17, 64, 40)
    items = [{"text": ("a",), "text_individual1": ("b",), "text_individual2": ("c",), "motion_lens": torch.tensor([t]),
              "cond": torch.randn(1, CW, generator=torch.Generator().manual_seed(i))} for i, t in enumerate(lens)]
    runs = {}
    for batching in ("sequential", "ragged"):
        gen, mm = generate_for_evaluation(model, items, max_length=64, mm_idxs=(1,), mm_num_repeats=3, batching=batching, seed=11)
        assert len(gen) == len(items) and len(mm) == 1 and mm[0]["mm_motions"].shape == (3, 64, 2, 262)
        runs[batching] = (gen, mm)
    for a, b in zip(runs["sequential"][0], runs["ragged"][0]):
        assert np.array_equal(a["motion1"], b["motion1"]) and np.array_equal(a["motion2"], b["motion2"])
    for a, b in zip(runs["sequential"][1], runs["ragged"][1]):
        assert np.array_equal(a["mm_motions"], b["mm_motions"])


# ---------------------------------------------------------------------------------------------------
# what stays refused
# ---------------------------------------------------------------------------------------------------
def test_ragged_calls_still_refused_by_name():
    from mixermdm_amd._lib import MMDMError
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict, synthetic_stats
    # the 4-way-CFG interaction sampler and the dual sampler
    sd = synthetic_state_dict(seed=7, std=0.05, bias_std=0.02, mixing_mode=4, **DIMS)
    for so, width, cw in ((2, 524, 3 * 768), (3, 524, 5 * 768)):
        pick = ("denoiser2.",) if so == 2 else ("denoiser1.", "denoiser2.")
        s = Sampler(d_heads=2, max_batch=4, max_frames=32, single_only=so, **{k: v for k, v in DIMS.items() if k.startswith("d_")})
        s.load_state_dict({k: v for k, v in sd.items() if k.startswith(pick)})
        s.prepare()
        s.set_schedule("ddim20")
        if so == 3:
            s.set_dual_weights("const", 0.5)
        cond, xs = inputs((8, 20), width=width, cw=cw, seed=2)
        with pytest.raises(MMDMError, match="ragged batches cover"):
            s.begin_ragged(cond, xs, (8, 20))
        s.close()
    # a key mask set on the handle (in2IN denoiser 1: the MDM handle takes no mask at all)
    st = synthetic_stats()
    s = Sampler(d_heads=2, m_heads=2, max_batch=4, max_frames=32, mixing_mode=4, **DIMS)
    s.load_state_dict(sd)
    s.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
    s.prepare()
    s.set_schedule("ddim20")
    s.set_key_mask(torch.ones(2, 20, dtype=torch.bool))
    cond, xs = inputs((8, 20), cw=8 * 768, seed=2)
    with pytest.raises(MMDMError, match="key mask"):
        s.begin_ragged(cond, xs, (8, 20))
    s.close()
    s = small(max_batch=4, max_frames=32)
    with pytest.raises(MMDMError, match="MDM"):
        s.set_key_mask(torch.ones(2, 20, dtype=torch.bool))
    s.close()
    # an MDM head size the ragged attention does not cover: D1 = 16, H1 = 2
    s = small(max_batch=4, max_frames=32, d1=(16, 32, 2, 2))
    cond, xs = inputs((8, 20), cw=6 * 768 + 2 * 16, seed=2)
    s.sample(cond[:1], xs[0][None])                      # the uniform call runs
    with pytest.raises(MMDMError, match="head size 8"):
        s.begin_ragged(cond, xs, (8, 20))
    s.close()
