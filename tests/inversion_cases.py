"""Shared by tests/test_inversion_cpu.py and tests/test_gpu_inversion.py: the five set-ups of tests/golden/inversion_*.npz (tests/golden/
make_golden_inversion.py) -- weights and inputs re-drawn from their seeds -- the float64 restatement of the reverse loop over the oracle, and the reverse
update as a float64 / numpy fp32 formula."""
import zlib
import numpy as np
import torch

BOUNDS = (2e-3, 3e-2)            # the project's loop bound (mean, 99th percentile)
CASES = ("full", "partial")
#          set-up        fixtures (fp32 everywhere; fp32_split on the second)       weight seeds
SETUPS = {"intergen": (("inversion_intergen", "inversion_intergen32"), dict(int=32)),
          "4way": (("inversion_4way", "inversion_4way32"), dict(int=31)),
          "dual": (("inversion_dual", "inversion_dual32"), dict(ind=30, int=31)),
          "individual": (("inversion_individual", "inversion_individual32"), dict(ind=30)),
          "mdm": (("inversion_mdm", "inversion_mdm128"), dict(ind=33))}
SCALES = {"intergen": dict(cfg_scale=3.5), "4way": dict(cfg_scale=3.0, cfg_scale_interaction=3.0, cfg_scale_individual=1.0),
          "dual": dict(cfg_scale_individual=2.0, cfg_scale_interaction=3.0), "individual": dict(cfg_scale=3.5), "mdm": dict(cfg_scale=2.5)}
COND_SLICES = {"intergen": 1, "4way": 3, "dual": 5, "individual": 1}
# (fixture, set-up, precision mode): fp32 at every size, fp32_split at the sizes its GEMMs take (latent 32 / ff 64; MDM: latent 128, head size 64)
PARITY = [(fx, su, "fp32") for su, (fxs, _) in SETUPS.items() for fx in fxs] + [(fxs[1], su, "fp32_split") for su, (fxs, _) in SETUPS.items()]


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def redraw(shapes, seed, std, prefix=""):
    """make_golden.reinit from names and shapes alone: every parameter randn(shape, Generator(crc32(name) + seed)) * std."""
    return {prefix + k: torch.randn(shp, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) + seed)) * std for k, shp in shapes.items()}


def dims(g):
    return int(g["latent_dim"]), int(g["ff_size"]), int(g["num_layers"]), int(g["H"])


def weights(g, setup, p_ind="denoiser1.", p_int="denoiser2."):
    """The set-up's parameters under the sampler's prefixes."""
    from mixermdm_amd.synthetic import denoiser_shapes, mdm_denoiser_shapes
    D, F, L, _ = dims(g)
    seeds, std = SETUPS[setup][1], float(g["wstd"])
    if setup == "mdm":
        return redraw(mdm_denoiser_shapes("", D, F, L), seeds["ind"], std, p_ind)
    W = {}
    if "ind" in seeds:
        W.update(redraw(denoiser_shapes("", D, F, L), seeds["ind"], std, p_ind))
    if "int" in seeds:
        W.update(redraw(denoiser_shapes("", D, F, L), seeds["int"], std, p_int))
    return W


def inputs(g, setup):
    """(motion [B, T, W], cond) of a fixture, from its seeds."""
    B, T, W = int(g["B"]), int(g["T"]), int(g["W"])
    s_motion, s_cond = [int(v) for v in g["seeds"]]
    cond = rnd(s_cond, B, int(g["latent_dim"])) if setup == "mdm" else rnd(s_cond, B, COND_SLICES[setup] * 768)
    return float(g["motion_scale"]) * rnd(s_motion, B, T, W), cond


def make_sampler(g, setup, precision="fp32", max_batch=None, max_frames=None, strategy=None):
    """The handle of a set-up, loaded, prepared and on the fixture's schedule."""
    from mixermdm_amd.sampler import Sampler
    D, F, L, H = dims(g)
    kind = {"intergen": dict(single_only=4, model2_kind=1), "4way": dict(single_only=4, cfg_form=1), "dual": dict(single_only=4, cfg_form=2),
            "individual": dict(single_only=1), "mdm": dict(single_only=1, model1_kind=1)}[setup]
    s = Sampler(d_latent=D, d_ff=F, d_layers=L, d_heads=H, max_batch=max_batch or int(g["B"]), max_frames=max_frames or int(g["T"]), precision=precision,
                **kind, **SCALES[setup])
    s.load_state_dict(weights(g, setup))
    s.prepare()
    s.set_schedule(strategy or str(g["strategy"]))
    if setup == "dual":
        s.set_dual_weights(str(g["w_func"]), float(g["w_value"]))
    return s


def oracle_x0(g, setup, W, x, t, cond):
    """The guidance wrapper's combined prediction at model timestep t, in the dtype of x (float64 in the tests)."""
    from oracle import mixer as M
    from oracle.denoiser import inter_denoiser
    from oracle.encoder import mdm_denoiser
    B, H, sc = x.shape[0], int(g["H"]), SCALES[setup]
    ts = torch.full((B,), int(t), dtype=torch.long)
    if setup in ("intergen", "mdm"):
        xx, tt, cc = torch.cat([x, x]), torch.cat([ts, ts]), torch.cat([cond, torch.zeros_like(cond)])
        out = inter_denoiser(W, "int.", xx, tt, cc, H) if setup == "intergen" else mdm_denoiser(W, "ind.", xx, tt, cc, H)
        return sc["cfg_scale"] * out[:B] + (1.0 - sc["cfg_scale"]) * out[B:]
    if setup == "individual":
        return M.cfg_single(W, "ind.", "individual", sc["cfg_scale"], x, ts, cond, H)
    if setup == "4way":
        return M.cfg_multiple(W, "int.", sc["cfg_scale"], sc["cfg_scale_interaction"], sc["cfg_scale_individual"], x, ts, cond, H)
    w = M.dual_weight(str(g["w_func"]), float(g["w_value"]), int(t))
    return M.cfg_dual(W, "ind.", "int.", sc["cfg_scale_individual"], sc["cfg_scale_interaction"], w, x, ts, cond, H)


def oracle_weights(g, setup):
    """float64 weights under "ind." / "int." with the oracle's pe buffers."""
    from oracle.layers import pe_table
    W = {k: v.double() for k, v in weights(g, setup, "ind.", "int.").items()}
    for p in ("ind.", "int."):
        if any(k.startswith(p) for k in W):
            W[p + "sequence_pos_encoder.pe"] = pe_table(int(g["latent_dim"])).double()
    return W


def oracle_reverse_loop(g, setup, k):
    """GaussianDiffusion.ddim_reverse_sample driven `for i in range(k)` (gaussian_diffusion.py:908-944) in float64 over the oracle's denoisers: float64
    tables throughout, as the reference's own float64 run has them.  -> (latent, last pred_xstart)."""
    from oracle.schedule import make_schedule
    sched = make_schedule("cosine", 1000, str(g["strategy"]))
    ab_next = np.append(sched.alphas_cumprod[1:], 0.0)
    W = oracle_weights(g, setup)
    x, cond = inputs(g, setup)
    x, cond = x.double(), cond.double()
    x0 = None
    for i in range(k):
        x0 = oracle_x0(g, setup, W, x, sched.timestep_map[i], cond)
        eps = (sched.sqrt_recip_alphas_cumprod[i] * x - x0) / sched.sqrt_recipm1_alphas_cumprod[i]
        x = x0 * np.sqrt(ab_next[i]) + np.sqrt(1.0 - ab_next[i]) * eps
    return x, x0


def reverse_update(x, x0, coef, rev, i, dtype):
    """One reverse update with the fp32 tables coef [4, S] / rev [2, S] as the kernel reads them, evaluated in `dtype` (np.float64: the yardstick;
    np.float32: the same formula in fp32, operation by operation)."""
    S = coef.shape[1]
    c0, c1, r0, r1 = (np.asarray(v, dtype=dtype) for v in (coef[0, i], coef[1, i], rev[0, i], rev[1, i]))
    x, x0 = np.asarray(x, dtype=dtype), np.asarray(x0, dtype=dtype)
    eps = (c0 * x - x0) / c1
    assert 0 <= i < S and eps.dtype == dtype
    return x0 * r0 + r1 * eps


def forward_update(x, x0, coef, i, dtype):
    """One forward (eta = 0) update with the same tables: rows 2 / 3 of coef instead of rev."""
    c0, c1, c2, c3 = (np.asarray(coef[r, i], dtype=dtype) for r in range(4))
    x, x0 = np.asarray(x, dtype=dtype), np.asarray(x0, dtype=dtype)
    return x0 * c2 + c3 * ((c0 * x - x0) / c1)
