"""CPU: the InterCLIP evaluator's fixture (tests/golden/evaluator.npz), the torch restatement the GPU tests lean on, the host-side refusals of
load_state_dict and the metric functions.  No compute entry point of the library is called here."""
import numpy as np
import pytest
import torch

import evaluator_cases as EC


@pytest.fixture(scope="module")
def g():
    return EC.fixture()


SMALL = ("int128", "int256", "ind128")


def test_redrawn_state_dict_is_the_recorded_one(g):
    from mixermdm_amd.evaluation import interclip_shapes, PE_KEY
    assert [str(c) for c in g["cases"]] == ["int128", "int256", "ind128", "full"]
    for case in g["cases"]:
        case = str(case)
        rec = dict(EC.case_names_shapes(g, case))
        assert PE_KEY in rec and rec[PE_KEY] == (2000, EC.case_cfg(g, case)["LATENT_DIM"])          # accepted and ignored: recomputed
        mine = interclip_shapes(EC.case_cfg(g, case), vocab=int(g["vocab"]), context=77)
        assert set(mine) == set(rec) - {PE_KEY}, set(mine) ^ set(rec)
        for k, s in mine.items():
            assert tuple(s) == rec[k], k
    W = EC.case_weights(g, "int128")
    assert {k: tuple(v.shape) for k, v in W.items()} == {k: s for k, s in EC.case_names_shapes(g, "int128") if not k.endswith(".pe")}


@pytest.mark.parametrize("case", SMALL)
def test_restatement_equals_the_reference_motion_encoder(g, case):
    """The padded torch restatement, in fp32 and in float64, against the reference's two runs: within YARD_FACTOR x |ref32 - ref64| quantile by quantile."""
    W, cfg = EC.case_weights(g, case), EC.case_cfg(g, case)
    motions, lens = EC.case_motions(g, case)
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            EC.yardstick(EC.encode_motion(W, cfg, motions, lens, dt), g[f"{case}:ref32"], g[f"{case}:ref64"], f"restatement {case} {dt}", report=False)


def test_restatement_equals_the_reference_text_encoder_and_wrapper_order(g):
    W = EC.case_weights(g, "int128")
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            EC.yardstick(EC.encode_text(W, g["text:tokens"], dt), g["text:ref32"], g["text:ref64"], f"restatement text {dt}", report=False)
        motions, lens = EC.case_motions(g, "int128")
        order = np.argsort(lens)[::-1].copy()
        assert np.array_equal(order, g["wrap:order"])
        me = EC.encode_motion(W, EC.case_cfg(g, "int128"), motions, lens, torch.float64)[torch.from_numpy(order)]
        te = EC.encode_text(W, g["wrap:tokens"], torch.float64)[torch.from_numpy(order)]
    EC.yardstick(me, g["wrap:motion_ref32"], g["wrap:motion_ref64"], "restatement wrapper motion", report=False)
    EC.yardstick(te, g["wrap:text_ref32"], g["wrap:text_ref64"], "restatement wrapper text", report=False)
    assert float(g["wrap:rank_gap"]) > 100 * float(g["wrap:max_err"])


def test_load_state_dict_refusals_are_raised_on_the_host(g):
    """Missing / unexpected / wrongly sized entries raise before anything is moved to a device (this box has none)."""
    from mixermdm_amd.evaluation import InterCLIP, strip_model_prefix, PE_KEY
    cfg = EC.case_cfg(g, "int128")
    sd = {k: torch.zeros(s) for k, s in EC.case_names_shapes(g, "int128")}
    assert PE_KEY in sd
    m = InterCLIP(cfg, device="cuda")
    bad = dict(sd)
    del bad["motion_encoder.out_ln.bias"]
    with pytest.raises(RuntimeError, match=r"Missing key\(s\): \['motion_encoder.out_ln.bias'\]"):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError, match=r"Unexpected key\(s\): \['motion_encoder.extra'\]"):
        m.load_state_dict(dict(sd, **{"motion_encoder.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"size mismatch for motion_encoder.embed_motion.weight: copying a param with shape \(128, 524\)"):
        m.load_state_dict(dict(sd, **{"motion_encoder.embed_motion.weight": torch.zeros(128, 524)}))
    with pytest.raises(RuntimeError, match="size mismatch for textTransEncoder.layers.7.linear1.weight"):
        m.load_state_dict(dict(sd, **{"textTransEncoder.layers.7.linear1.weight": torch.zeros(2048, 768)}))
    with pytest.raises(RuntimeError, match="no weights loaded"):
        m.encode_motion({"motions": torch.zeros(1, 4, 524), "motion_lens": [4]})
    with pytest.raises(ValueError, match="INPUT_DIM"):
        InterCLIP(dict(cfg, INPUT_DIM=262))
    with pytest.raises(ValueError, match="MODE"):
        InterCLIP(dict(cfg, MODE="both"))
    with pytest.raises(ValueError, match="item 2 has motion_lens = 0"):
        m.sequence_layout(40, [3, 1, 0])
    off, ln, total, longest = m.sequence_layout(40, [17, 1, 33, 16, 50])
    assert ln.tolist() == [18, 2, 34, 17, 41] and off.tolist() == [0, 18, 20, 54, 71] and total == 112 and longest == 41
    ck = strip_model_prefix({"model.motion_encoder.out.bias": 1, "model.latent_scale": 2, "out.bias": 3})
    assert ck == {"motion_encoder.out.bias": 1, "latent_scale": 2, "out.bias": 3}


def test_eval_yaml_is_the_full_size_case(g):
    import os
    from mixermdm_amd.configs import get_config
    cfg = get_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "eval.yaml"))
    full = EC.case_cfg(g, "full")
    for k in ("MODE", "LATENT_DIM", "NUM_HEADS", "FF_SIZE", "NUM_LAYERS", "INPUT_DIM", "ACTIVATION"):
        assert cfg[k] == full[k], k


def test_metric_functions_equal_the_recorded_results(g):
    from mixermdm_amd import evaluation as E
    (sa, *sha), (sb, *shb), (sm, *shm) = [[int(v) for v in r] for r in g["met:in"]]
    a, b = EC.rnd(sa, *sha).double().numpy(), EC.rnd(sb, *shb).double().numpy()
    mm = EC.rnd(sm, *shm).double().numpy().reshape(6, 8, 16)
    rt = dict(rtol=1e-9, atol=0)
    dist = E.euclidean_distance_matrix(a[:32], b[:32])
    np.testing.assert_allclose(dist, g["met:dist"], **rt)
    top = E.calculate_top_k(np.argsort(dist, axis=1), 3)
    assert top.dtype == bool and np.array_equal(top, g["met:top_k"])
    assert np.array_equal(E.calculate_R_precision(a[:32], b[:32], 3, sum_all=True), g["met:r_precision"])
    assert np.array_equal(E.calculate_R_precision(a[:32], b[:32], 3), g["met:top_k"])
    np.testing.assert_allclose(E.calculate_matching_score(a, b), g["met:matching"], **rt)
    np.testing.assert_allclose(E.calculate_matching_score(a, b, sum_all=True), g["met:matching"].sum(), **rt)
    mu, cov = E.calculate_activation_statistics(a)
    np.testing.assert_allclose(mu, g["met:mu"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(cov, g["met:cov"], rtol=1e-9, atol=1e-15)
    fid = E.calculate_frechet_distance(*E.calculate_activation_statistics(b), mu, cov)
    assert abs(fid - float(g["met:fid"])) <= float(g["met:fid_rtol"]) * abs(float(g["met:fid"])), (fid, float(g["met:fid"]))
    assert float(g["met:fid_rtol"]) >= 1e-10
    s_div, s_mm = [int(v) for v in g["met:seeds"]]
    np.random.seed(s_div)
    np.testing.assert_allclose(E.calculate_diversity(a, 20), g["met:diversity"], **rt)
    np.random.seed(s_mm)
    np.testing.assert_allclose(E.calculate_multimodality(mm, 5), g["met:multimodality"], **rt)
    with pytest.raises(AssertionError):
        E.calculate_diversity(a[:20], 20)


def test_ops_of_the_evaluator_refuse_cpu_tensors():
    from mixermdm_amd import ops
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.l2_normalize(torch.zeros(2, 8), torch.ones(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.motion_pack(torch.zeros(2, 4, 524), z, z, 3, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.motion_tokens_(torch.zeros(6, 8), torch.zeros(8), torch.zeros(4, 8), z, z, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.encoder_layer_ragged_(torch.zeros(6, 128), {k: torch.zeros(1) for k in
                                  ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight",
                                   "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")}, 2, z, z, 3)
