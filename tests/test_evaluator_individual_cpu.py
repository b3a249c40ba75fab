"""CPU: the InterCLIP individual evaluator -- the restatement (oracle.geometry centring + evaluator_cases encoder) against the reference's own
EvaluatorModelWrapperIndividual (tests/golden/evaluator_individual.npz), the wrapper's host logic over a fake model, the replication summary and the
F-score against numpy expressions, the refusals and the config file."""
import os
import numpy as np
import pytest
import torch

import evaluator_cases as EC
import evaluator_individual_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return IC.fixture()


# ---- the restatement against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ind128", "ind256"])
def test_restatement_matches_the_reference_wrapper(g, case):
    assert g[f"{case}:motion_ref32"].shape == (8, 512) and int(g["shape"][0]) == 4          # per-call batch 4, never 3
    EC.yardstick(IC.restated_embeddings(g, case, torch.float32), g[f"{case}:motion_ref32"], IC.restated_embeddings(g, case, torch.float64),
                 f"individual restatement {case}", report=False)


@pytest.mark.parametrize("case", ["ind128", "ind256"])
def test_interleaved_text_order_is_the_recorded_one(g, case):
    from mixermdm_amd.evaluation import EvaluatorModelWrapperIndividual as W
    t1, t2 = ["1:%d" % i for i in range(4)], ["2:%d" % i for i in range(4)]
    assert W._text_batch((None, None, None, None, None, t1, t2))["text"] == [str(v) for v in g[f"{case}:text_order"]]


def test_seeded_persons_restate_inside_the_geometry_rule():
    """The claim the GPU comparisons rest on: at the listed seeds the fp32 restatement has no element outside GEO of its float64 run."""
    for seed in IC.SEEDS:
        for m in (IC.person(seed), IC.zero_tails(IC.person(seed), IC.LENS)):
            frac, worst = IC.outside(IC.center_ih(m, torch.float32), IC.center_ih(m, torch.float64), **IC.GEO)
            assert frac == 0.0 and worst <= 6.5e-5, (seed, frac, worst)


# ---- the wrapper's host logic ---------------------------------------------------------------------------------------------------------------
class FakeModel:
    """Stands where an InterCLIP stands: records what the wrapper hands the two encoders."""
    cfg = {"MODE": "individual", "EXTENDED": True}
    device = torch.device("cpu")
    mode = "individual"

    def __init__(self):
        self.calls = []

    def encode_motion_individual(self, batch):
        self.calls.append(("motion", batch))
        batch["motion_emb"] = torch.zeros(2 * batch["motions"].shape[0], 512)
        return batch

    def encode_text(self, batch):
        self.calls.append(("text", batch))
        n = len(batch["text"]) if "text" in batch else batch["tokens_text"].shape[0]
        batch["text_emb"] = torch.arange(n, dtype=torch.float32)[:, None].expand(n, 512)
        return batch


def _wrapper(model):
    from mixermdm_amd.evaluation import EvaluatorModelWrapperIndividual
    w = object.__new__(EvaluatorModelWrapperIndividual)
    w.model, w.cfg, w.device, w.extended = model, model.cfg, model.device, True
    return w


def test_wrapper_hands_over_both_persons_unsorted_and_interleaved_texts():
    m = FakeModel()
    w = _wrapper(m)
    m1, m2 = EC.rnd(1, 3, 6, 262), EC.rnd(2, 3, 6, 262)
    lens = torch.tensor([2, 6, 4])
    te, me = w.get_co_embeddings((["a", "b", "c"], ["x"] * 3, m1, m2.numpy(), lens, ("p0", "p1", "p2"), ["q0", "q1", "q2"]))
    (_, mb), (_, tb) = m.calls
    assert torch.equal(mb["motions"], torch.cat([m1, m2], dim=-1)) and mb["motions"].dtype == torch.float32          # no length sort, no slicing
    assert mb["motion_lens"].tolist() == [2, 6, 4]
    assert tb["text"] == ["p0", "q0", "p1", "q1", "p2", "q2"]
    assert te.shape == (6, 512) and me.shape == (6, 512) and te[:, 0].tolist() == [0, 1, 2, 3, 4, 5]          # the text embeddings are not reordered
    assert w.individual is True


def test_wrapper_interleaves_token_rows():
    m = FakeModel()
    w = _wrapper(m)
    t1, t2 = torch.arange(12).reshape(3, 4), 100 + torch.arange(12).reshape(3, 4)
    w.get_co_embeddings((None, None, torch.zeros(3, 5, 262), torch.zeros(3, 5, 262), np.array([5, 5, 1]), t1, t2.numpy()))
    tok = m.calls[1][1]["tokens_text"]
    assert torch.equal(tok, torch.stack([t1[0], t2[0], t1[1], t2[1], t1[2], t2[2]]))


def test_wrapper_refusals():
    from mixermdm_amd.evaluation import EvaluatorModelWrapperIndividual, InterCLIP
    m = FakeModel()
    w = _wrapper(m)
    five = (None, ["x"] * 2, torch.zeros(2, 5, 262), torch.zeros(2, 5, 262), torch.tensor([5, 3]))
    with pytest.raises(ValueError, match="EXTENDED"):
        w.get_co_embeddings(five)
    with pytest.raises(ValueError, match="EXTENDED"):
        w.get_co_embeddings(five + (None, None))
    assert not m.calls                                                       # refused before anything is encoded
    assert w.get_motion_embeddings(five).shape == (4, 512)                   # the motion side needs no text
    cfg = {"INPUT_DIM": 258, "ACTIVATION": "gelu", "LATENT_DIM": 128, "FF_SIZE": 256, "NUM_LAYERS": 2, "NUM_HEADS": 2, "MODE": "interaction"}
    inter = InterCLIP(cfg, device="cpu")
    with pytest.raises(ValueError, match="'interaction'"):
        inter.encode_motion_individual({"motions": torch.zeros(1, 4, 524), "motion_lens": [4]})
    with pytest.raises(ValueError, match="'interaction'"):
        EvaluatorModelWrapperIndividual(inter)


def test_evaluate_generated_builds_the_seven_tuples():
    from mixermdm_amd import evaluation as E
    seen = []

    class Rec:
        individual = True

        def get_co_embeddings(self, batch):
            seen.append(batch)
            n = 2 * len(batch[2])
            e = torch.eye(n, 512)
            return e, e

        def get_motion_embeddings(self, batch):
            return torch.eye(2 * len(batch[2]), 512)

    items = [{"motion1": np.zeros((4, 262)), "motion2": np.ones((4, 262)), "motion_lens": torch.tensor(4 - i), "text": "t", "text_individual1": ("a%d" % i,),
              "text_individual2": ("b%d" % i,)} for i in range(4)]
    res = E.evaluate_generated(Rec(), items, batch_size=2, diversity_times=2)
    assert [len(b) for b in seen] == [7, 7] and seen[0][5] == [("a0",), ("a1",)] and seen[0][6] == [("b0",), ("b1",)] and seen[0][4].tolist() == [4, 3]
    assert res["r_precision"].tolist() == [1.0, 1.0, 1.0] and res["mm_dist"] == 0.0          # 8 embeddings: every metric over 2B per batch
    tok = [dict(d, tokens_individual1=torch.full((5,), i), tokens_individual2=torch.full((5,), 10 + i)) for i, d in enumerate(items)]
    seen.clear()
    E.evaluate_generated(Rec(), tok, batch_size=4, diversity_times=2)
    assert torch.equal(seen[0][5], torch.tensor([[0] * 5, [1] * 5, [2] * 5, [3] * 5])) and torch.equal(seen[0][6][:, 0], torch.tensor([10, 11, 12, 13]))


# ---- replications and the F-score -------------------------------------------------------------------------------------------------------------
def test_summaries_against_numpy():
    from mixermdm_amd.evaluation import summarize_replications, f_score_summary
    rng = np.random.RandomState(11)
    reps = lambda: [{"mm_dist": float(rng.rand() + 3), "r_precision": rng.rand(3), "fid": float(rng.rand() + 5), "diversity": float(rng.rand()),
                     "multimodality": float(rng.rand())} for _ in range(5)]
    ra, rb = reps(), reps()
    sa, sb = summarize_replications(ra), summarize_replications(rb)
    rt = dict(rtol=1e-12, atol=0)
    for k in ("mm_dist", "r_precision", "fid", "diversity", "multimodality"):
        va, vb = np.array([d[k] for d in ra]), np.array([d[k] for d in rb])
        np.testing.assert_allclose(sa[k]["mean"], va.sum(axis=0) / 5, **rt)
        np.testing.assert_allclose(sa[k]["conf_interval"], 1.96 * np.sqrt(((va - va.sum(axis=0) / 5) ** 2).sum(axis=0) / 5) / np.sqrt(5), **rt)
        ma, mb = va.sum(axis=0) / 5, vb.sum(axis=0) / 5
        f = f_score_summary(sa, sb)[k]
        np.testing.assert_allclose(f["f_score"], 2 * ma * mb / (ma + mb), **rt)
        np.testing.assert_allclose(f["conf_interval"], (sa[k]["conf_interval"] + sb[k]["conf_interval"]) / 2, **rt)
    assert sa["r_precision"]["mean"].shape == (3,) and f_score_summary(sa, sb)["r_precision"]["f_score"].shape == (3,) and np.ndim(sa["fid"]["mean"]) == 0
    # a metric that a replication could not form (diversity: None) is left out, and so is one that only one side holds
    ra[2]["diversity"] = None
    s2 = summarize_replications(ra)
    assert "diversity" not in s2 and "diversity" not in f_score_summary(s2, sb) and set(f_score_summary(s2, sb)) == set(s2)
    with pytest.raises(ValueError):
        summarize_replications([])


# ---- refusals and the config file -------------------------------------------------------------------------------------------------------------
def test_new_ops_refuse_cpu_tensors():
    from mixermdm_amd import ops
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.center_motion(torch.zeros(2, 4, 524))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.center_motion(torch.zeros(2, 4, 262), npers=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.center_pack(torch.zeros(2, 4, 524), z, z, 5, 20, 272)


def test_individual_config_differs_in_mode_only():
    from mixermdm_amd.configs import get_config as load
    a, b = load(os.path.join(ROOT, "configs", "eval.yaml")), load(os.path.join(ROOT, "configs", "eval_individual.yaml"))
    assert a["MODE"] == "interaction" and b["MODE"] == "individual"
    assert {k: v for k, v in dict(a).items() if k != "MODE"} == {k: v for k, v in dict(b).items() if k != "MODE"}


def test_f_score_of_two_zero_means_is_zero():
    from mixermdm_amd.evaluation import f_score_summary
    z = {"r_precision": {"mean": np.array([0.0, 0.5, 1.0]), "conf_interval": np.zeros(3)}}
    np.testing.assert_array_equal(f_score_summary(z, z)["r_precision"]["f_score"], [0.0, 0.5, 1.0])
