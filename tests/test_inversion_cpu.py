"""CPU: DDIM inversion without a GPU -- the reverse table against the reference's fp32 rows, a float64 restatement of the reverse loop over the oracle's
denoisers against the reference's recorded float64 latents (tests/golden/inversion_*.npz, tests/golden/make_golden_inversion.py), the fixtures' own
figures, and the argument rules of the Python layer (steps, start_step, packing, batching)."""
import numpy as np
import pytest
import torch

import inversion_cases as IC


def test_reverse_coefficients_are_the_references_rows_bitwise(golden):
    """The fixture keeps the reference's fp32 radicands (the gathered ab_next and 1 - ab_next: exact operations, the same bits on every platform) and its
    th.sqrt of them.  The table is held BITWISE to the correctly rounded fp32 sqrt of the radicands -- what numpy and the GPU's th.sqrt give -- as
    test_intergen_cpu.py holds the eta table to np.sqrt of its recorded radicand; the builder's CPU th.sqrt is 1 ulp off IEEE for ~0.6 % of inputs (two of
    ddim4's four entries), so the recorded th.sqrt rows are held to 1 ulp, and bitwise at the exact endpoints (0, 1)."""
    from mixermdm_amd.schedule import make_schedule
    g, _, _ = golden("inversion_schedule")
    for strat, S in (("ddim4", 4), ("ddim50", 50)):
        sch = make_schedule("cosine", 1000, strat)
        rev = sch.reverse_coefficients()
        assert rev.shape == (2, S) and rev.dtype == np.float32
        assert g[f"{strat}:ab_next"].dtype == np.float32 and g[f"{strat}:one_minus_ab_next"].dtype == np.float32
        np.testing.assert_array_equal(rev[0], np.sqrt(g[f"{strat}:ab_next"]))
        np.testing.assert_array_equal(rev[1], np.sqrt(g[f"{strat}:one_minus_ab_next"]))
        for row, key in ((rev[0], "sqrt_ab_next"), (rev[1], "sqrt_one_minus_ab_next")):
            ulps = np.abs(row.view(np.int32).astype(np.int64) - g[f"{strat}:{key}"].view(np.int32).astype(np.int64))
            print(f"{strat} {key}: {int((ulps != 0).sum())} of {S} entries differ from the recorded th.sqrt, by at most {int(ulps.max())} ulp")
            assert ulps.max() <= 1 and ulps[-1] == 0
        assert rev[0, S - 1] == 0.0 and rev[1, S - 1] == 1.0
        # the level a reverse step at i arrives at, ab[i + 1], is the level the forward step at i + 2 arrives at (ab_prev[i + 2]): the same float64 entry
        coef = sch.device_coefficients()
        np.testing.assert_array_equal(rev[0, :-2], coef[2, 2:])
        np.testing.assert_array_equal(rev[1, :-2], coef[3, 2:])


@pytest.mark.parametrize("setup", list(IC.SETUPS))
def test_fixture_figures_and_redrawn_weights(golden, setup):
    for fx in IC.SETUPS[setup][0]:
        g, _, _ = golden(fx)
        B, T, W = int(g["B"]), int(g["T"]), int(g["W"])
        assert (B, str(g["strategy"]), T, W) == (2, "ddim4", 12 if setup == "mdm" else 20, 524 if setup in ("intergen", "4way", "dual") else 262)
        np.testing.assert_array_equal(g["bounds"], np.array(IC.BOUNDS))
        for name, k in zip(IC.CASES, (4, 2)):
            assert int(g[f"case:{name}"]) == k
            lat, px, l64 = g[f"{name}:latent"], g[f"{name}:pred_xstart"], g[f"{name}:latent_f64"]
            assert lat.shape == px.shape == l64.shape == (B, T, W) and lat.dtype == px.dtype == np.float32 and l64.dtype == np.float64
            for tag in ("latent", "pred_xstart"):
                err, ratio = g[f"{name}:{tag}:ref_f64_err"], g[f"{name}:{tag}:ref_f64_ratio"]
                np.testing.assert_allclose(err / np.array(IC.BOUNDS), ratio, rtol=1e-12)
                assert ratio.max() <= 0.25, (fx, name, tag, ratio)
            d = np.abs(lat.astype(np.float64) - l64)
            np.testing.assert_allclose([d.mean(), np.percentile(d, 99)], g[f"{name}:latent:ref_f64_err"], rtol=1e-12)
    # the weights are the existing fixtures' draws: intergen_standalone.npz, single.npz and mdm.npz store the latent-16 sets
    g, _, _ = golden(IC.SETUPS[setup][0][0])
    have = {"intergen": ("intergen_standalone", "ig.", "denoiser2."), "individual": ("single", "ind.", "denoiser1."), "mdm": ("mdm", "mdm.", "denoiser1.")}.get(setup)
    if have is not None:
        _, w, _ = golden(have[0])
        W = IC.weights(g, setup)
        stored = w(have[1])
        assert {have[2] + k for k in stored} == set(W)
        assert all(torch.equal(W[have[2] + k], v) for k, v in stored.items())


@pytest.mark.parametrize("fixture,setup", [(fx, su) for fx, su, prec in IC.PARITY if prec == "fp32"])
def test_restated_reverse_loop_lands_on_the_recorded_float64_latents(golden, fixture, setup):
    """Two float64 evaluations of one loop differ by summation order only: ~1e-13 of the values' size after two blocks and four steps.  Held to 1e-9 of the
    latent's largest value -- five orders below the reference's own fp32 rounding (ref_f64_err), so an index or table slip cannot pass."""
    g, _, _ = golden(fixture)
    for name in IC.CASES:
        lat, px = IC.oracle_reverse_loop(g, setup, int(g[f"case:{name}"]))
        want = torch.from_numpy(g[f"{name}:latent_f64"])
        d = float((lat - want).abs().max())
        print(f"{fixture} {name}: |oracle f64 - reference f64| max {d:.3e} (|latent| max {float(want.abs().max()):.1f})")
        assert d <= 1e-9 * float(want.abs().max()), (fixture, name, d)
        dp = (px - torch.from_numpy(g[f"{name}:pred_xstart"]).double()).abs().numpy()
        rec = g[f"{name}:pred_xstart:ref_f64_err"]
        assert dp.mean() <= 1.05 * rec[0] + 1e-12 and np.percentile(dp, 99) <= 1.05 * rec[1] + 1e-12, (fixture, name)


def test_reverse_then_forward_formula_returns_to_the_start():
    """The algebraic identity the GPU test rests on, in float64 on the fp32 tables: with a constant x0, k < S reverse updates from step 0 (levels ab[0] -> ab[k]) followed by
    the forward updates k .. 1 return x -- up to the fp32 rounding of the reference's tables: sqrt(1 - ab_prev[1]) is taken from fp32(1 - ab[0]) = 4.2e-5 with an
    absolute error of 2^-24, 7e-4 relative after the root, on a term of size |x - x0| ~ 1 (measured: 5.3e-4 for every k).  A shifted row misses by 0.16 .. 3."""
    from mixermdm_amd.schedule import make_schedule
    rng = np.random.default_rng(5)
    x_in, x0 = 0.5 * rng.standard_normal((7, 262)), 0.3 * rng.standard_normal((1, 262))
    for strat, ks in (("ddim4", (1, 2, 3)), ("ddim20", (7,))):
        sch = make_schedule("cosine", 1000, strat)
        coef, rev = sch.device_coefficients(), sch.reverse_coefficients()
        for k in ks:
            x = x_in
            for i in range(k):
                x = IC.reverse_update(x, x0, coef, rev, i, np.float64)
            for i in range(k, 0, -1):
                x = IC.forward_update(x, x0, coef, i, np.float64)
            assert np.abs(x - x_in).max() <= 2e-3, (strat, k, np.abs(x - x_in).max())
            wrong = x_in
            for i in range(k):
                wrong = IC.reverse_update(wrong, x0, coef, np.roll(rev, 1, axis=1), i, np.float64)
            for i in range(k, 0, -1):
                wrong = IC.forward_update(wrong, x0, coef, i, np.float64)
            assert np.abs(wrong - x_in).max() > 0.1, (strat, k)


def test_steps_and_start_step_rules():
    from mixermdm_amd.sampler import invert_steps, check_start_step
    assert invert_steps(None, 4) == 4 and invert_steps(1, 4) == 1 and invert_steps(np.int64(4), 4) == 4
    for bad in (0, 5, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match=r"outside \[1, 4\]"):
            invert_steps(bad, 4)
    assert check_start_step(0, 4) == 0 and check_start_step(3, 4) == 3
    for bad in (-1, 4, 1.5, True, None):
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            check_start_step(bad, 4)
    with pytest.raises(ValueError, match="exclusive with init_image / skip_timesteps"):
        check_start_step(2, 4, skip_timesteps=1)
    with pytest.raises(ValueError, match="exclusive with init_image / skip_timesteps"):
        check_start_step(2, 4, init_image=torch.zeros(1))


def test_packing_rule():
    from mixermdm_amd.models import pack_groups
    assert pack_groups([2, 1], [10, 30]) == [[(0, 0), (0, 1), (1, 0)]]
    assert pack_groups([2, 1], [10, 30], max_rows=45) == [[(0, 0), (0, 1)], [(1, 0)]]
    assert pack_groups([3], [10], max_items=2) == [[(0, 0), (0, 1)], [(0, 2)]]
    assert pack_groups([1, 1], [100, 5], max_rows=50) == [[(0, 0)], [(1, 0)]]          # a motion longer than max_rows is a group of its own
    assert pack_groups([], []) == []


def tiny_cfg(**over):
    from mixermdm_amd.configs import CfgNode
    c = dict(NAME="InterGen", LATENT_DIM=16, FF_SIZE=32, NUM_LAYERS=2, NUM_HEADS=2, INPUT_DIM=262, CFG_WEIGHT=3.5, STRATEGY="ddim4", DIFFUSION_STEPS=1000,
             BETA_SCHEDULER="cosine", W_FUNC="exp", W_VALUE=0.004)
    c.update(over)
    return CfgNode(c)


def test_facade_argument_rules():
    """Checked before any device is touched (the models are on the CPU: a call that got past validation raises "MI355X only")."""
    from mixermdm_amd.models import InterGen, MDM, in2IN
    ig, md = InterGen(tiny_cfg()), MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=2.5))
    b = lambda W=524, cw=768, **kw: dict(cond=torch.zeros(1, cw), motions=torch.zeros(1, 8, W), **kw)
    with pytest.raises(ValueError, match="gives no 'motions'"):
        ig.invert(dict(cond=torch.zeros(1, 768)))
    with pytest.raises(ValueError, match=r"motions \[B, T, 524\] expected"):
        ig.invert(dict(cond=torch.zeros(1, 768), motions=torch.zeros(8, 524)))
    with pytest.raises(ValueError, match=r"x_T \[1, 8, 524\] expected"):
        ig.invert(b(W=262))
    with pytest.raises(ValueError, match="batching 'inflight' not recognized"):
        ig.invert_many([b()], batching="inflight")
    with pytest.raises(RuntimeError, match="MI355X only"):
        ig.invert(b())
    with pytest.raises(RuntimeError, match="MI355X only"):
        ig.invert_many([b(), b()], batching="ragged", steps=2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        md.invert(b(W=262, cw=16))
    with pytest.raises(ValueError, match=r"x_T \[1, 8, 262\] expected"):
        md.invert_many([b(W=524, cw=16)])
    for mode, W in (("individual", 262), ("interaction", 524), ("dual", 524)):
        m = in2IN(tiny_cfg(NAME="in2IN"), mode)
        conds = {k: torch.zeros(1, 768) for k in ("cond_interaction", "cond_interaction_individual1", "cond_interaction_individual2",
                                                   "cond_individual_individual1", "cond_individual_individual2")}
        with pytest.raises(RuntimeError, match="MI355X only"):
            m.invert(dict(conds, motions=torch.zeros(1, 8, W)))
        with pytest.raises(ValueError, match=rf"x_T \[1, 8, {W}\] expected"):
            m.invert_many([dict(conds, motions=torch.zeros(1, 8, W + 1))], batching="sequential")
