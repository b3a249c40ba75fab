"""GPU: the InterCLIP evaluator (mixermdm_amd/evaluation.py) -- the ragged post-norm encoder layer, the three row kernels in both builds, both
encoders against the reference's fixture (tests/golden/evaluator.npz) by the float64 yardstick, the bitwise batch-independence of a motion
embedding, the wrapper's order convention and the evaluation pass."""
import numpy as np
import pytest
import torch

import evaluator_cases as EC
import rowop_cases as RC
from parity_tol import YARD_FACTOR, YARD_FLOOR, record

pytestmark = pytest.mark.gpu

LENS = (34, 33, 18, 17, 2)          # token sequences of the fixture's lengths 33, 32, 17, 16, 1: both sides of the 16-key chunk edges
_MODELS = {}


@pytest.fixture(scope="module")
def g():
    return EC.fixture()


def model_of(g, case):
    from mixermdm_amd.evaluation import InterCLIP
    if case not in _MODELS:
        sd = dict(EC.case_weights(g, case))
        D = EC.case_cfg(g, case)["LATENT_DIM"]
        sd["motion_encoder.sequence_pos_encoder.pe"] = torch.zeros(2000, D)          # the buffer of a real checkpoint: accepted, ignored
        _MODELS[case] = InterCLIP(EC.case_cfg(g, case), device="cuda:0").load_state_dict(sd, strict=True)
    return _MODELS[case]


def seqs(lens, gap=0, dev="cuda:0"):
    """Packed sequences, `gap` unowned rows in front of the third one: (seq_off, seq_len int32 device tensors, offsets, total rows)."""
    off, o = [], 0
    for i, n in enumerate(lens):
        o += gap if i == 2 else 0
        off.append(o)
        o += n
    return torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev), off, o


# ---- 1. the ragged encoder layer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,H", [("int128", 2), ("int256", 2)])
def test_ragged_encoder_layer_is_bitwise_the_layer_on_each_sequence_alone(g, case, H):
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    W = EC.case_weights(g, case)
    D = EC.case_cfg(g, case)["LATENT_DIM"]
    p = "motion_encoder.transformer.layers.0."
    w = {k.replace("self_attn.", ""): W[p + k].cuda().contiguous() for k in
         ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight", "linear1.bias",
          "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")}
    so, sl, off, total = seqs(LENS, gap=3)
    x0 = EC.rnd(31, total, D).cuda()
    x0[off[2] - 3:off[2]] = float("nan")          # rows outside every sequence influence nothing
    x = ops.encoder_layer_ragged_(x0.clone(), w, H, so, sl, max(LENS))
    for o, n in zip(off, LENS):
        alone = ops.encoder_layer_(x0[o:o + n][None].clone(), w, H)[0]
        assert torch.isfinite(alone).all() and torch.equal(x[o:o + n], alone), (case, n)
    # a longer max_len only sizes the grid
    assert torch.equal(ops.encoder_layer_ragged_(x0.clone(), w, H, so, sl, 40)[:off[2] - 3], x[:off[2] - 3])
    with pytest.raises(MMDMError, match="head size 8 is not supported") as e:
        ops.encoder_layer_ragged_(x0.clone(), w, D // 8, so, sl, max(LENS))
    assert e.value.status == 4
    with pytest.raises(MMDMError, match="norm_first is not supported") as e:
        ops.encoder_layer_ragged_(x0.clone(), w, H, so, sl, max(LENS), norm_first=True)
    assert e.value.status == 4


# ---- 2. the row kernels, both builds, against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("npers", [2, 1])
def test_motion_pack_is_the_index_expression(build, npers):
    from mixermdm_amd import ops
    lens = (34, 33, 18, 17, 2, 41)                                     # the last item fills the buffer: 40 frames
    C, Tpad = npers * 262, 40
    store = torch.full((len(lens), Tpad + 4, C + 4), float("nan"))       # a strided view: row stride C + 4, item stride (Tpad + 4)(C + 4)
    src = RC.rnd(50 + npers, len(lens), Tpad, C)
    for i, n in enumerate(lens):
        store[i, :n - 1, :C] = src[i, :n - 1]                            # frames at and beyond the length stay NaN: never read
    so, sl, off, total = seqs(lens, gap=3)
    kp = (npers * 258 + 15) // 16 * 16
    out = torch.full((total + 2, kp), -77.0, device="cuda:0")
    ops.motion_pack(store.cuda()[:, :Tpad, :C], so, sl, max(lens), total, npers=npers, k_pad=kp, build=build, out=out)
    ref = torch.full((total + 2, kp), -77.0, dtype=torch.float64)
    for i, (o, n) in enumerate(zip(off, lens)):
        ref[o:o + n] = 0.0
        ref[o + 1:o + n, :npers * 258] = src[i, :n - 1].double().reshape(n - 1, npers, 262)[..., :258].reshape(n - 1, -1)
    assert torch.equal(out.cpu().double(), ref), (build, npers)          # a copy: exact; unowned rows and the rows behind the last untouched


@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("D", [128, 260, 1024])
def test_motion_tokens_is_one_rounded_add(build, D):
    from mixermdm_amd import ops
    lens = (34, 33, 18, 17, 2)
    so, sl, off, total = seqs(lens, gap=3)
    h0, q, pe = RC.rnd(60, total, D), RC.rnd(61, 1, D), EC.pe_table(D, 2000)
    h = ops.motion_tokens_(h0.cuda(), q.cuda(), pe.cuda(), so, sl, max(lens), build=build)
    ref = h0.double().clone()
    for o, n in zip(off, lens):
        ref[o] = q[0].double() + pe[0].double()
        ref[o + 1:o + n] = h0[o + 1:o + n].double() + pe[1:n].double()
    # one fp32 addition is the correctly rounded float64 sum of the same two fp32 values
    assert torch.equal(h.cpu(), ref.float()), (build, D)


def l2_bound(x, ref):
    """fp32 sum of D squares in any order: at most D roundings of 2^-24 relative to the (all-positive) sum, halved by the square root; the square root,
    the division and the scaling add one rounding each; the scale itself is exact (one fp32 value)."""
    D = x.shape[-1]
    return (D / 2 + 4) * 2.0 ** -24 * ref.abs() + 1e-37


@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("D", [4, 252, 512, 516, 1024, 2048])
def test_l2_normalize_against_float64(build, D):
    from mixermdm_amd import ops
    x, _ = RC.norm_rows(85, D, seed=70)
    x[0] = 1.0                                                          # (row 0 of norm_rows is all zeros: 0 / 0 in the reference too)
    scale = torch.tensor([0.37])
    got = ops.l2_normalize(x.cuda(), scale.cuda(), build=build).cpu()
    ref = x.double() / x.double().norm(dim=-1, keepdim=True) * scale.double()
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all() and bool((err <= l2_bound(x, ref)).all()), (build, D, float((err / l2_bound(x, ref)).max()))
    # a row's bits do not depend on how many rows the launch has
    for r in (0, 4, 84):
        assert torch.equal(ops.l2_normalize(x[r:r + 1].cuda(), scale.cuda(), build=build).cpu()[0], got[r]), (build, D, r)
    if build == 0:
        assert torch.equal(ops.l2_normalize(x.reshape(5, 17, D).cuda(), scale.cuda()).cpu().reshape(85, D), got)


# ---- 3. / 5. the encoders against the fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["int128", "int256", "ind128", "full"])
def test_encode_motion_against_the_reference(g, case):
    m = model_of(g, case)
    motions, lens = EC.case_motions(g, case)
    got = m.encode_motion({"motions": motions, "motion_lens": torch.tensor(lens)})["motion_emb"]
    assert got.shape == (len(lens), 512) and got.is_cuda
    EC.yardstick(got, g[f"{case}:ref32"], g[f"{case}:ref64"], f"evaluator encode_motion {case}")
    if case == "full":
        _MODELS.pop(case)          # 110 M floats: not kept for the rest of the session


def test_encode_text_against_the_reference(g):
    m = model_of(g, "int128")
    got = m.encode_text({"tokens_text": g["text:tokens"]})["text_emb"]
    EC.yardstick(got, g["text:ref32"], g["text:ref64"], "evaluator encode_text")


# ---- 4. bitwise properties ---------------------------------------------------------------------------------------------------------------
def test_motion_embedding_does_not_depend_on_the_batch(g):
    m = model_of(g, "int128")
    motions, lens = EC.case_motions(g, "int128")
    enc = lambda mo, ln: m.encode_motion({"motions": mo, "motion_lens": torch.tensor(ln)})["motion_emb"]
    ref = enc(motions, lens)
    for i, n in enumerate(lens):          # alone (in its own, shorter buffer too)
        assert torch.equal(enc(motions[i:i + 1], [n])[0], ref[i]), i
        assert torch.equal(enc(motions[i:i + 1, :n].contiguous(), [n])[0], ref[i]), i
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(enc(motions[perm], [lens[i] for i in perm]), ref[perm])
    poisoned = motions.clone()
    for i, n in enumerate(lens):
        poisoned[i, n:] = float("nan")
    assert torch.equal(enc(poisoned, lens), ref) and torch.isfinite(ref).all()
    with pytest.raises(ValueError, match="item 1 has motion_lens = 0"):
        enc(motions[:2], [4, 0])


# ---- 6. the wrapper and the evaluation pass -----------------------------------------------------------------------------------------------
def test_wrapper_order_and_evaluation_pass(g):
    from mixermdm_amd.evaluation import EvaluatorModelWrapper, evaluate_generated
    wr = EvaluatorModelWrapper(model_of(g, "int128"))
    motions, lens = EC.case_motions(g, "int128")
    tokens = torch.from_numpy(g["wrap:tokens"])
    names = ["n%d" % i for i in range(5)]
    te, me = wr.get_co_embeddings((names, tokens, motions[..., :262], motions[..., 262:], torch.tensor(lens)))
    EC.yardstick(te, g["wrap:text_ref32"], g["wrap:text_ref64"], "evaluator wrapper text_emb")
    EC.yardstick(me, g["wrap:motion_ref32"], g["wrap:motion_ref64"], "evaluator wrapper motion_emb")
    order = np.argsort(lens)[::-1].copy()
    assert np.array_equal(order, g["wrap:order"])
    assert torch.equal(wr.get_motion_embeddings((names, None, motions[..., :262].numpy(), motions[..., 262:].numpy(), np.array(lens))), me)
    alone = wr.model.encode_motion({"motions": motions, "motion_lens": lens})["motion_emb"]
    assert torch.equal(alone[torch.from_numpy(order).cuda()], me)
    generated = [{"motion1": motions[i, :, :262].numpy(), "motion2": motions[i, :, 262:].numpy(), "motion_lens": torch.tensor(lens[i]),
                  "tokens_text": tokens[i]} for i in range(5)]
    mm = [{"mm_motions": motions[:3].reshape(3, 40, 2, 262).numpy(), "motion_lens": torch.tensor(16)}] * 2
    np.random.seed(3)
    res = evaluate_generated(wr, generated, mm_generated=mm, groundtruth=generated[::-1], diversity_times=3, mm_num_times=2)
    # the R-precision counts of the reference's own embeddings, exactly: the smallest gap between neighbouring distances (rank_gap) is > 100 x
    # the reference's fp32 error, so nothing within the yardstick of it can swap two ranks
    assert np.array_equal(np.rint(res["r_precision"] * 5).astype(int), g["wrap:top_k"]), (res["r_precision"], g["wrap:top_k"])
    d_got, d_ref = float(abs(float(res["mm_dist"]) - float(g["wrap:mm_dist64"]))), abs(float(g["wrap:mm_dist32"]) - float(g["wrap:mm_dist64"]))
    print(f"mm_dist {res['mm_dist']:.9f}: |got - f64| {d_got:.3e}, |ref32 - f64| {d_ref:.3e}")
    record("evaluator mm_dist", kind="evaluator_yardstick", got_vs_f64=d_got, ref32_vs_f64=d_ref, factor=YARD_FACTOR, floor=YARD_FLOOR)
    assert d_got <= YARD_FACTOR * d_ref + YARD_FLOOR
    assert abs(res["fid"]) < 1e-6 and res["diversity"] > 0 and res["multimodality"] > 0          # the same set as its own ground truth


# ---- 7. from the generation loop to the scores ----------------------------------------------------------------------------------------------
def test_generated_motions_are_scored_end_to_end(g, tmp_path, golden):
    """generate_for_evaluation -> evaluate_generated on the tiny model of test_gpu_facade.  The tiny model's head size is not one the ragged attention
    kernels cover (64 / 128): batching="ragged" is refused by name there, asserted below, so its three items go through the sequential loop -- the lists
    handed over have the same layout either way."""
    from test_gpu_facade import tiny_model
    from mixermdm_amd._lib import MMDMError
    from mixermdm_amd.generation import generate_for_evaluation
    from mixermdm_amd.evaluation import EvaluatorModelWrapper, evaluate_generated
    m, gm, t = tiny_model(tmp_path, golden, strategy="ddim20")
    cond = t("cfg_cond")[:1].cuda()
    tokens = torch.from_numpy(g["wrap:tokens"])
    items = [dict(text=("a",), text_individual1=("b",), text_individual2=("c",), motion_lens=torch.tensor([T]), cond=cond) for T in (8, 16, 10)]
    with pytest.raises(MMDMError, match=r"head size 8 \(the ragged attention kernels cover 64 and 128\)"):
        generate_for_evaluation(m, items, max_length=16, mm_idxs=[1], mm_num_repeats=3, batching="ragged")
    gen, mm = generate_for_evaluation(m, items, max_length=16, mm_idxs=[1], mm_num_repeats=3, batching="sequential")
    for i, d in enumerate(gen):
        d["tokens_text"] = tokens[i]
    res = evaluate_generated(EvaluatorModelWrapper(model_of(g, "int128")), gen, mm_generated=mm, groundtruth=gen, diversity_times=2, mm_num_times=2)
    assert set(res) == {"mm_dist", "r_precision", "fid", "diversity", "multimodality"} and res["r_precision"].shape == (3,)
    assert all(np.isfinite(np.asarray(v, dtype=float)).all() for v in res.values()), res
    assert len(gen) == 3 and len(mm) == 1 and mm[0]["mm_motions"].shape == (3, 16, 2, 262)
    assert 0 <= res["r_precision"][0] <=res["r_precision"][1] <= res["r_precision"][2] <= 1
