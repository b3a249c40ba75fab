"""GPU: the InterCLIP individual evaluator -- the two centring entries (ops.center_motion / ops.center_pack) against the reference's vectors and the
float64 restatement, the floor over the whole buffer, the fused operand bitwise against center_motion + motion_pack, InterCLIP.encode_motion_individual
against the reference's own EvaluatorModelWrapperIndividual (tests/golden/evaluator_individual.npz) by the float64 yardstick, its bitwise batch
independence, and the evaluation pass with both wrappers up to the F-score summary."""
import numpy as np
import pytest
import torch

import evaluator_cases as EC
import evaluator_individual_cases as IC
from test_gpu_evaluator import seqs
from test_gpu_kernels import assert_close

pytestmark = pytest.mark.gpu

GEO = IC.GEO
_MODELS, _EMB = {}, {}


@pytest.fixture(scope="module")
def g():
    return IC.fixture()


def model_of(g, case):
    from mixermdm_amd.evaluation import InterCLIP
    if case not in _MODELS:
        _MODELS[case] = InterCLIP(EC.case_cfg(g, case), device="cuda:0").load_state_dict(dict(EC.case_weights(g, case)), strict=True)
    return _MODELS[case]


def embeddings_of(g, case):
    """encode_motion_individual of the fixture batch, computed once (tests 5 and 7 hold the same tensor)."""
    if case not in _EMB:
        motions, lens = IC.case_motions(g, case)
        _EMB[case] = model_of(g, case).encode_motion_individual({"motions": motions, "motion_lens": torch.tensor(lens)})["motion_emb"]
    return _EMB[case]


# ---- 1. center_motion against the reference's vectors -----------------------------------------------------------------------------------------
def test_center_motion_against_the_reference_vectors(golden):
    from mixermdm_amd import ops
    _, _, t = golden("geometry")
    for a, b in [("rand_a", "rand_b"), ("valid_c", "valid_d")]:
        m = torch.cat([t(a), t(b)], -1).cuda()
        out = ops.center_motion(m)
        assert_close(out[..., :262], t(a + ":center_ih"), what=a, **GEO)
        assert_close(out[..., 262:], t(b + ":center_ih"), what=b, **GEO)
        one = ops.center_motion(t(b).cuda(), npers=1)
        assert_close(one, t(b + ":center_ih"), what=b + " alone", **GEO)
        for o in (out[..., 258:262], out[..., 520:524], one[..., 258:262]):
            assert torch.count_nonzero(o).item() == 0                   # exactly zero
        assert torch.equal(one, out[..., 262:])                          # a person's bits do not depend on its neighbour


# ---- 2. center_motion against the float64 restatement -------------------------------------------------------------------------------------------
# (B, T) -> the persons of the shape: (seed, lengths beyond which the frames are zeroed, or None for a live tail).  (4, 24): the four seeds, both tails.
# The other shapes take the listed seeds whose fp32 restatement is inside GEO with frac = 0 (asserted below, on the CPU): at (3, 13) seeds 14 and 20; at
# (2, 47) NO listed seed is with a live tail (4.1e-5 .. 8.1e-5 of the elements outside), so that shape runs zeroed tails only -- seed 15 with lengths
# (47, 3) and seed 20 with (47, 20); item 0 keeps all 47 x 22 joints live in both.
L424, L313 = (24, 17, 1, 9), (13, 5, 1)
PERSONS = {
    (4, 24): [(s, tail) for tail in (L424, None) for s in IC.SEEDS],
    (1, 1): [(s, None) for s in IC.SEEDS],
    (3, 13): [(14, L313), (20, L313), (14, None), (20, None)],          # B = 3: the last-dimension cross product against the oracle
    (2, 47): [(15, (47, 3)), (20, (47, 20))],                            # 47 x 22 is no multiple of the block size
}


@pytest.mark.parametrize("shape", list(PERSONS))
def test_center_motion_against_float64(shape):
    from mixermdm_amd import ops
    B, T = shape
    ps, refs = [], []
    for seed, tail in PERSONS[shape]:
        m = IC.person(seed, B, T)
        m = m if tail is None else IC.zero_tails(m, tail)
        r64 = IC.center_ih(m, torch.float64)
        frac, worst = IC.outside(IC.center_ih(m, torch.float32), r64, **GEO)
        print(f"center_motion {shape} seed {seed} tail {tail}: fp32 restatement outside {frac:.2e}, max {worst:.2e}")
        assert frac == 0.0, (shape, seed, tail, frac)                    # the reference side uses none of GEO's allowance
        ps.append(m)
        refs.append(r64)
    for m, r64 in zip(ps, refs):
        got = ops.center_motion(m.cuda(), npers=1)
        assert_close(got, r64, what=f"npers 1 {shape}", **GEO)
        assert torch.count_nonzero(got[..., 258:]).item() == 0
    for k in range(0, len(ps), 2):
        got = ops.center_motion(torch.cat(ps[k:k + 2], -1).cuda(), npers=2)
        assert_close(got, torch.cat(refs[k:k + 2], -1), what=f"npers 2 {shape}", **GEO)
        assert torch.count_nonzero(got[..., 258:262]).item() == 0 and torch.count_nonzero(got[..., 520:]).item() == 0


# ---- 3. the floor spans the buffer ---------------------------------------------------------------------------------------------------------------
def test_floor_is_taken_over_the_whole_buffer():
    from mixermdm_amd import ops
    m = IC.person(7)                                                     # live tails
    m[1, 20, 3 * 5 + 1] = -50.0                                          # Y of joint 5 in a frame beyond item 1's length of 17
    got = ops.center_motion(m.cuda(), npers=1).cpu()
    whole, cut = IC.center_ih(m, torch.float64), IC.center_ih(m[:, :17], torch.float64)
    assert_close(got[1, :17], whole[1, :17], what="valid frames, floor over the buffer", **GEO)
    assert float((got[1, :17].double() - cut[1]).abs().max()) > 40.0     # the buffer cut to the length stands 50 lower


# ---- 4. center_pack is motion_pack of center_motion -----------------------------------------------------------------------------------------------
def test_center_pack_is_bitwise_motion_pack_of_center_motion():
    from mixermdm_amd import ops
    B, T, kp = 4, 24, 272
    m = torch.cat([IC.person(7), IC.person(14)], -1).cuda()              # live tails
    lens = [1 + n for n in L424 for _ in (0, 1)]                         # token sequences: p1 of item 0, p2 of item 0, ...
    so, sl, off, total = seqs(lens, gap=3)
    centred = ops.center_motion(m).reshape(B, T, 2, 262).transpose(1, 2).reshape(2 * B, T, 262).contiguous()
    nan = lambda: torch.full((total + 2, kp), float("nan"), device="cuda:0")
    ref = ops.motion_pack(centred, so, sl, max(lens), total, npers=1, k_pad=kp, out=nan())
    got = ops.center_pack(m, so, sl, max(lens), total, k_pad=kp, out=nan())
    bits = lambda x: x.view(torch.int32)
    assert torch.equal(bits(got), bits(ref))
    owned = torch.zeros(total + 2, dtype=torch.bool)
    for o, n in zip(off, lens):
        owned[o:o + n] = True
        assert torch.count_nonzero(bits(got[o])).item() == 0            # the token row: +0.0
        assert torch.isfinite(got[o + 1:o + n, :258]).all()
    assert torch.count_nonzero(bits(got[owned.cuda()][:, 258:])).item() == 0          # columns [258, Kp): +0.0
    assert torch.isnan(got[(~owned).cuda()]).all() and int((~owned).sum()) == 5      # the gap and the rows behind the last keep their NaN
    # beyond a length only position Y is ever read (the floor)
    poisoned = m.clone()
    y = torch.zeros(524, dtype=torch.bool)
    for p in (0, 262):
        y[p + 1:p + 66:3] = True
    for i, n in enumerate(L424):
        poisoned[i, n:, ~y.cuda()] = float("nan")
    assert torch.equal(bits(ops.center_pack(poisoned, so, sl, max(lens), total, k_pad=kp, out=nan())), bits(got))


# ---- 5. embeddings against the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ind128", "ind256"])
def test_individual_embeddings_against_the_reference(g, case):
    got = embeddings_of(g, case)
    assert got.shape == (8, 512) and got.is_cuda
    EC.yardstick(got, g[f"{case}:motion_ref32"], IC.restated_embeddings(g, case, torch.float64), f"evaluator encode_motion_individual {case}")


# ---- 6. bitwise batch independence -----------------------------------------------------------------------------------------------------------------
def test_individual_embeddings_do_not_depend_on_the_batch(g):
    m = model_of(g, "ind128")
    motions, lens = IC.case_motions(g, "ind128")
    enc = lambda mo, ln: m.encode_motion_individual({"motions": mo, "motion_lens": torch.tensor(ln)})["motion_emb"]
    ref = embeddings_of(g, "ind128")
    assert torch.isfinite(ref).all()
    for i, n in enumerate(lens):
        assert torch.equal(enc(motions[i:i + 1], [n]), ref[2 * i:2 * i + 2]), i
    perm = [2, 0, 3, 1]
    assert torch.equal(enc(motions[perm], [lens[i] for i in perm]), ref.reshape(4, 2, 512)[perm].reshape(8, 512))
    with pytest.raises(ValueError, match="item 1 has motion_lens = 0"):
        enc(motions[:2], [4, 0])


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_both_wrappers_score_generated_motions_up_to_the_f_score(g, tmp_path, golden):
    from test_gpu_facade import tiny_model
    from mixermdm_amd.generation import generate_for_evaluation
    from mixermdm_amd.evaluation import (EvaluatorModelWrapper, EvaluatorModelWrapperIndividual, evaluate_generated, summarize_replications,
                                         f_score_summary)
    import test_gpu_evaluator as TE
    ge = EC.fixture()
    wi = EvaluatorModelWrapperIndividual(model_of(g, "ind128"))
    # the fixture batch through the wrapper: bitwise the encoders' own results, in the interleaved order
    motions, lens = IC.case_motions(g, "ind128")
    tok1, tok2 = torch.from_numpy(g["ind128:tokens1"]), torch.from_numpy(g["ind128:tokens2"])
    batch = (["n%d" % i for i in range(4)], None, motions[..., :262], motions[..., 262:].numpy(), torch.tensor(lens), tok1, tok2.numpy())
    te, me = wi.get_co_embeddings(batch)
    assert torch.equal(me, embeddings_of(g, "ind128")) and torch.equal(wi.get_motion_embeddings(batch[:5]), me)
    inter = torch.stack([tok1, tok2], dim=1).reshape(8, -1)
    assert torch.equal(te, wi.model.encode_text({"tokens_text": inter})["text_emb"])
    EC.yardstick(te, g["ind128:text_ref32"], EC.encode_text(EC.case_weights(g, "ind128"), inter, torch.float64), "evaluator individual wrapper text_emb")
    # generated motions, scored by both wrappers
    m, _, t = tiny_model(tmp_path, golden, strategy="ddim20")
    cond = t("cfg_cond")[:1].cuda()
    items = [dict(text=("a",), text_individual1=("b",), text_individual2=("c",), motion_lens=torch.tensor([T]), cond=cond) for T in (8, 16, 10)]
    gen, mm = generate_for_evaluation(m, items, max_length=16, mm_idxs=[1], mm_num_repeats=3, batching="sequential")
    assert all(d["text_individual1"] == "b" and d["text_individual2"] == "c" for d in gen)
    wtok = torch.from_numpy(ge["wrap:tokens"])
    for i, d in enumerate(gen):
        d.update(tokens_text=wtok[i], tokens_individual1=tok1[i], tokens_individual2=tok2[i])
    gt = [dict(d, motion1=1.1 * d["motion1"], motion2=1.1 * d["motion2"]) for d in gen]          # another set: a Frechet distance above zero
    ww = EvaluatorModelWrapper(TE.model_of(ge, "int128"))
    np.random.seed(5)
    reps = {k: [evaluate_generated(w, gen, mm_generated=mm, groundtruth=gt, diversity_times=2, mm_num_times=2) for _ in range(2)]
            for k, w in (("interaction", ww), ("individual", wi))}
    keys = {"mm_dist", "r_precision", "fid", "diversity", "multimodality"}
    for res in reps["interaction"] + reps["individual"]:
        assert set(res) == keys and res["r_precision"].shape == (3,) and 0 <= res["r_precision"][0] <= res["r_precision"][2] <= 1
    sums = {k: summarize_replications(v) for k, v in reps.items()}
    f = f_score_summary(sums["interaction"], sums["individual"])
    assert set(f) == keys
    for k in keys:
        shape = (3,) if k == "r_precision" else ()
        for d, names in ((sums["interaction"][k], ("mean", "conf_interval")), (sums["individual"][k], ("mean", "conf_interval")),
                         (f[k], ("f_score", "conf_interval"))):
            for nm in names:
                assert np.shape(d[nm]) == shape and np.isfinite(d[nm]).all(), (k, nm, d[nm])
