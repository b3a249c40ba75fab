"""CPU: host side of the sampler options (eta > 0, init_image / skip_timesteps, x_start): the eta tables against the reference's values
(tests/golden/sampler_opts.npz, tests/golden/make_golden_sampler_opts.py), the generator's definition in numpy against the published known
answers, and the loop arguments that stay refused."""
import numpy as np
import pytest

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox4x32-10 from its definition (Salmon et al., SC'11), vectorised: ctr [..., 4], key [..., 2] unsigned 32-bit -> [..., 4]."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = [np.asarray(key)[..., k].astype(np.uint64) for k in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack(c, -1).astype(np.uint32)


def step_normal_f64(seed, loop_pos, B, T):
    """float64 evaluation of the sampler's step noise [B, T, 524] (include/mmdm.h: mmdm_randn_f32) from the same integer draws."""
    b, t, col = np.meshgrid(np.arange(B), np.arange(T), np.arange(524), indexing="ij")
    ctr = np.stack([t * 524 + col, b, np.full_like(b, loop_pos), np.zeros_like(b)], -1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    r = philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    u1 = ((r[..., 0] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((r[..., 1] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def test_numpy_philox_reproduces_the_known_answers():
    """The three known-answer vectors of Philox4x32-10 (Random123's kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    z = step_normal_f64(1234, 1, 2, 40)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02


def test_eta_tables_are_the_references_bitwise(golden):
    """sigma and the radicand 1 - ab_prev - sigma^2 are the reference's own fp32 tensors, bit for bit; the table's first row is the radicand's
    correctly rounded fp32 root.  The reference's th.sqrt of it is NOT compared bitwise: the CPU fp32 sqrt of the torch build that wrote the fixture
    is not correctly rounded -- at eta = 0.5, step 1 it returns 0x3bb6641f where the IEEE root (numpy's, and float64's rounded once) is 0x3bb66420 --
    while the rows the kernels have always read come from numpy (device_coefficients, tests/test_abi_cpu.py), and the eta = 0 identity below ties the
    new table to those.  It is held within one ulp instead."""
    from mixermdm_amd.schedule import make_schedule
    g, _, _ = golden("sampler_opts")
    sch = make_schedule("cosine", 1000, str(g["strategy"]))
    for eta in (0.5, 1.0):
        tab = sch.eta_coefficients(eta)
        assert tab.dtype == np.float32 and tab.shape == (2, sch.num_timesteps)
        np.testing.assert_array_equal(tab[1], g[f"eta{eta}:sigma"])
        np.testing.assert_array_equal((np.float32(1) - sch.alphas_cumprod_prev.astype(np.float32)) - tab[1] * tab[1], g[f"eta{eta}:c3_arg"])
        np.testing.assert_array_equal(tab[0], np.sqrt(g[f"eta{eta}:c3_arg"]))
        ulps = np.abs(tab[0].view(np.int32).astype(np.int64) - g[f"eta{eta}:c3"].view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, ulps
        assert tab[1][0] == 0 and (tab[1][1:] > 0).all()                # no variance left at the last step
    for strat in ("ddim4", "ddim50"):
        sch = make_schedule("cosine", 1000, strat)
        co, tab = sch.device_coefficients(), sch.eta_coefficients(0.0)
        assert tab[0].tobytes() == co[3].tobytes()                       # eta = 0: the plain update's coefficient, bit for bit
        assert tab[1].tobytes() == np.zeros(sch.num_timesteps, np.float32).tobytes()
    a, b = sch.q_sample_coefficients(10)
    assert a == np.float32(np.sqrt(sch.alphas_cumprod[10])) and b == np.float32(np.sqrt(1.0 - sch.alphas_cumprod[10]))


def test_fixture_cases_are_well_conditioned(golden):
    """Every stored case: the reference's own fp32 run within a quarter of the loop bounds of its float64 run (the generator refuses others)."""
    g, _, _ = golden("sampler_opts")
    names = [k[5:] for k in g if k.startswith("case:")]
    assert sorted(names) == ["all", "eta", "init", "init0", "pin", "skip"]
    for n in names:
        assert g[f"{n}:ref_f64_ratio"].max() <= 0.25, n
        assert g[f"{n}:output"].shape == (2, 20, 524)


def test_loop_arguments_that_stay_refused():
    """Raised before any device work, as before the options existed."""
    from mixermdm_amd.models import MixerDiffusion
    from mixermdm_amd.schedule import get_named_beta_schedule, space_timesteps
    d = MixerDiffusion(space_timesteps(1000, "ddim4"), betas=get_named_beta_schedule("cosine", 1000))
    shape = (1, 4, 524)
    for kw in (dict(dump_steps=[1]), dict(const_noise=True)):
        with pytest.raises(NotImplementedError):
            d.ddim_sample_loop(None, shape, clip_denoised=False, **kw)
    for kw in (dict(clip_denoised=True), dict(denoised_fn=lambda x: x), dict(cond_fn=lambda *a: 0), dict(randomize_class=True), dict(cond_fn_with_grad=True)):
        kw.setdefault("clip_denoised", False)
        with pytest.raises(NotImplementedError, match="clip_denoised=False, eta=0, no guidance fn"):
            d.ddim_sample_loop(None, shape, eta=0.5, x_start=object(), **kw)
    with pytest.raises(ValueError, match="not both"):
        d.ddim_sample_loop(None, shape, clip_denoised=False, eta=0.5, step_noise=object(), seed=1)
    with pytest.raises(ValueError, match="eta"):
        d.ddim_sample_loop(None, shape, clip_denoised=False, eta=-1.0)
