"""GPU: the InterCLIP evaluator in the fp32_split precision mode (mixermdm_amd/evaluation.py).
  1. the plane-writing pack kernels are bitwise ops.split_f32 of the fp32 forms (motion_pack in both builds, center_pack); unowned rows untouched
  2. the plane-writing motion_tokens: fp32 rows bitwise ops.motion_tokens_, planes bitwise split_f32 of them
  3. the ragged split layer is bitwise the uniform split layer on every sequence alone; its refusals by name; the uniform layer at head size 96 (the fp32
     attention inside the split layer) against float64 with the fp32 layer as yardstick
  4. split embeddings against the reference's fixtures by the unchanged float64 yardstick AND by the sharper rule -- relative RMS and max |emb - ref64| /
     max |ref64| at most 3 x the project's fp32 evaluator on the same inputs + 1e-6 (factor and floor of test_gpu_mask_split.py (b) / parity_tol.YARD_FACTOR)
  5. bitwise batch independence in split mode; precision="fp32" is the default constructor bit for bit
  6. the wrapper's exact R-precision counts and one evaluation pass with a split wrapper.
Measured on an MI355X (sharper rule, split / fp32 evaluator, relative RMS and scaled max): see DESIGN 9c."""
import numpy as np
import pytest
import torch

import evaluator_cases as EC
import evaluator_individual_cases as IC
import rowop_cases as RC
from parity_tol import YARD_FACTOR, YARD_FLOOR, record
from test_gpu_evaluator import seqs

pytestmark = pytest.mark.gpu

LENS = (34, 33, 18, 17, 2)          # both sides of the 16-key chunk edges
PACK_LENS = (34, 33, 18, 17, 2, 41)          # the last item fills the 40-frame buffer
_MODELS = {}
_LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight", "linear1.bias",
               "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
bits16 = lambda x: x.contiguous().view(torch.int16)
bits32 = lambda x: x.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def g():
    return EC.fixture()


@pytest.fixture(scope="module")
def gi():
    return IC.fixture()


def model_of(fx, case, precision, tag=""):
    """InterCLIP of a fixture case; precision None = the default constructor."""
    from mixermdm_amd.evaluation import InterCLIP
    key = (tag, case, precision)
    if key not in _MODELS:
        kw = {} if precision is None else {"precision": precision}
        _MODELS[key] = InterCLIP(EC.case_cfg(fx, case), device="cuda:0", **kw).load_state_dict(dict(EC.case_weights(fx, case)), strict=True)
    return _MODELS[key]


def owned_rows(off, lens, rows):
    own = torch.zeros(rows, dtype=torch.bool)
    for o, n in zip(off, lens):
        own[o:o + n] = True
    return own.cuda()


def planes_buffer(rows, ld, fill=7.0):
    return torch.full((2, rows * ld), fill, device="cuda:0", dtype=torch.float16)


# ---- 1. the pack kernels write split_f32 of the fp32 form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("npers", [2, 1])
def test_motion_pack_planes_are_split_f32_of_the_fp32_form(build, npers):
    from mixermdm_amd import ops
    C, Tpad = npers * 262, 40
    kp = ops.split_k_pad(npers)
    assert kp == (544, 288)[npers == 1]
    store = torch.full((len(PACK_LENS), Tpad + 4, C + 4), float("nan"))       # a strided view; frames at and beyond a length stay NaN: never read
    src = RC.rnd(50 + npers, len(PACK_LENS), Tpad, C)
    src[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-9, 60000.0])                  # zeros of both signs, below the lo plane's reach, near the fp16 limit
    for i, n in enumerate(PACK_LENS):
        store[i, :n - 1, :C] = src[i, :n - 1]
    so, sl, off, total = seqs(PACK_LENS, gap=3)
    motions = store.cuda()[:, :Tpad, :C]
    a = ops.motion_pack(motions, so, sl, max(PACK_LENS), total, npers=npers, k_pad=kp, build=build, out=torch.full((total + 2, kp), -77.0, device="cuda:0"))
    buf = planes_buffer(total + 2, kp)
    ret = ops.motion_pack_split(motions, so, sl, max(PACK_LENS), total, npers=npers, k_pad=kp, build=build, out=buf)
    pl = buf.view(2, total + 2, kp)
    assert ret.shape == (2, total, kp) and ret.data_ptr() == buf.data_ptr()
    own = owned_rows(off, PACK_LENS, total + 2)
    want = ops.split_f32(a)
    assert torch.equal(bits16(pl[:, own]), bits16(want[:, own])), (build, npers)
    assert bool((pl[:, ~own] == 7.0).all()) and int((~own).sum()) == 5      # the gap and the rows behind the last: untouched
    for o, n in zip(off, PACK_LENS):
        assert torch.count_nonzero(bits16(pl[:, o])).item() == 0             # token rows: +0 in both planes
    assert torch.count_nonzero(bits16(pl[:, own][:, :, npers * 258:])).item() == 0          # pad columns: +0 in both planes
    assert torch.isfinite(pl[:, own].float()).all()


def test_center_pack_planes_are_split_f32_of_the_fp32_form():
    from mixermdm_amd import ops
    L424 = (24, 17, 1, 9)
    kp = ops.split_k_pad(1)
    m = torch.cat([IC.person(7), IC.person(14)], -1).cuda()              # live tails
    lens = [1 + n for n in L424 for _ in (0, 1)]
    so, sl, off, total = seqs(lens, gap=3)
    a = ops.center_pack(m, so, sl, max(lens), total, k_pad=kp, out=torch.full((total + 2, kp), -77.0, device="cuda:0"))
    buf = planes_buffer(total + 2, kp)
    ops.center_pack_split(m, so, sl, max(lens), total, k_pad=kp, out=buf)
    pl = buf.view(2, total + 2, kp)
    own = owned_rows(off, lens, total + 2)
    want = ops.split_f32(a)
    assert torch.equal(bits16(pl[:, own]), bits16(want[:, own]))
    assert bool((pl[:, ~own] == 7.0).all()) and int((~own).sum()) == 5
    for o in off:
        assert torch.count_nonzero(bits16(pl[:, o])).item() == 0
    assert torch.count_nonzero(bits16(pl[:, own][:, :, 258:])).item() == 0
    # the planes hold the values: hi + lo / 2048 is the fp32 operand to 2^-22 relative (a tiny absolute floor below 2^-14)
    back = pl[0, own].double() + pl[1, own].double() / 2048
    assert bool(((back - a[own].double()).abs() <= 2.0 ** -22 * a[own].double().abs() + 2.0 ** -36).all())


# ---- 2. the token rows and their planes in one pass --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [0, 1])
@pytest.mark.parametrize("D", [128, 260, 1024])
def test_motion_tokens_split_rows_and_planes(build, D):
    from mixermdm_amd import ops
    so, sl, off, total = seqs(PACK_LENS, gap=3)
    h0, q, pe = RC.rnd(60, total + 2, D).cuda(), RC.rnd(61, 1, D).cuda(), EC.pe_table(D, 2000).cuda()
    ref = ops.motion_tokens_(h0.clone(), q, pe, so, sl, max(PACK_LENS), build=build)
    buf = planes_buffer(total + 2, D)
    h, pl = ops.motion_tokens_split_(h0.clone(), q, pe, so, sl, max(PACK_LENS), build=build, planes=buf)
    assert torch.equal(bits32(h), bits32(ref)), (build, D)               # every row: the owned ones rewritten alike, the others as they were
    own = owned_rows(off, PACK_LENS, total + 2)
    assert torch.equal(bits16(pl[:, own]), bits16(ops.split_f32(h)[:, own])), (build, D)
    assert bool((pl[:, ~own] == 7.0).all())


# ---- 3. the split layer ---------------------------------------------------------------------------------------------------------------------------
def layer_weights(g, case):
    W = EC.case_weights(g, case)
    p = "motion_encoder.transformer.layers.0."
    return {k.replace("self_attn.", ""): W[p + k].cuda().contiguous() for k in _LAYER_KEYS}


@pytest.mark.parametrize("case,H", [("int128", 2), ("int256", 2)])
def test_ragged_split_layer_is_bitwise_the_uniform_split_layer_on_each_sequence(g, case, H):
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    D = EC.case_cfg(g, case)["LATENT_DIM"]
    assert D // H in (64, 128)
    w = layer_weights(g, case)
    ws = ops.encoder_layer_split_weights(w)
    assert ws["packed"] and ws["in_proj_weight"].shape == (2, 3 * D, D) and ws["in_proj_weight"].dtype == torch.float16
    so, sl, off, total = seqs(LENS, gap=3)
    x0 = EC.rnd(31, total, D).cuda()
    x0[off[2] - 3:off[2]] = float("nan")          # rows outside every sequence influence nothing
    for last in (False, True):
        x, xs = x0.clone(), ops.split_f32(x0)
        ops.encoder_layer_ragged_split_(x, xs, ws, H, so, sl, max(LENS), last=last)
        for o, n in zip(off, LENS):
            a, as_ = x0[o:o + n][None].clone(), ops.split_f32(x0[o:o + n][None])
            ops.encoder_layer_split_(a, as_, ws, H, last=last)
            assert torch.isfinite(a).all() and torch.equal(bits32(x[o:o + n]), bits32(a[0])), (case, n, last)
            assert torch.equal(bits16(xs[:, o:o + n]), bits16(as_[:, 0])), (case, n, last)
            if not last:
                assert torch.equal(bits16(xs[:, o:o + n]), bits16(ops.split_f32(x[o:o + n]))), (case, n)          # the planes are those of the rows
        # a longer max_len only sizes the grid
        y, ys = x0.clone(), ops.split_f32(x0)
        ops.encoder_layer_ragged_split_(y, ys, ws, H, so, sl, 40, last=last)
        own = owned_rows(off, LENS, total)
        assert torch.equal(bits32(y[own]), bits32(x[own])) and torch.equal(bits16(ys[:, own]), bits16(xs[:, own]))
    # plain planes and fragment order: the same bits
    wp = ops.encoder_layer_split_weights(w, pack=False)
    assert not wp["packed"]
    z, zs = x0.clone(), ops.split_f32(x0)
    ops.encoder_layer_ragged_split_(z, zs, wp, H, so, sl, max(LENS), last=True)
    assert torch.equal(bits32(z[own]), bits32(x[own]))
    # close to the fp32 layer (the accuracy proper is held on the embeddings, below)
    f = ops.encoder_layer_ragged_(x0.clone(), w, H, so, sl, max(LENS))
    assert float((x[own] - f[own]).abs().max()) < 1e-4 * float(f[own].abs().max())
    fresh = lambda: (x0.clone(), ops.split_f32(x0))
    with pytest.raises(MMDMError, match="head size 8 is not supported") as e:
        ops.encoder_layer_ragged_split_(*fresh(), ws, D // 8, so, sl, max(LENS))
    assert e.value.status == 4
    with pytest.raises(MMDMError, match="norm_first is not supported") as e:
        ops.encoder_layer_ragged_split_(*fresh(), ws, H, so, sl, max(LENS), norm_first=True)
    assert e.value.status == 4
    with pytest.raises(MMDMError, match="norm_first is not supported") as e:
        a = x0[:LENS[0]][None].clone()
        ops.encoder_layer_split_(a, ops.split_f32(a), ws, H, norm_first=True)
    assert e.value.status == 4


def random_layer(D, F, seed, dtype=torch.float32):
    """A post-norm layer's weights under the names of evaluator_cases._encoder_layer (prefix "l.")."""
    shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,), "self_attn.out_proj.weight": (D, D), "self_attn.out_proj.bias": (D,),
              "linear1.weight": (F, D), "linear1.bias": (F,), "linear2.weight": (D, F), "linear2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,),
              "norm2.weight": (D,), "norm2.bias": (D,)}
    W = {}
    for i, (k, s) in enumerate(shapes.items()):
        r = EC.rnd(seed + i, *s)
        W["l." + k] = ((1.0 + 0.1 * r) if k in ("norm1.weight", "norm2.weight") else r * (0.1 if len(s) == 1 else (1.0 / s[1]) ** 0.5)).to(dtype)
    return W


def _dist(got, ref64):
    """(relative RMS, max |got - ref64| / max |ref64|) in float64."""
    got, ref64 = torch.as_tensor(np.asarray(got.detach().cpu()) if torch.is_tensor(got) else got).double(), torch.as_tensor(ref64).double()
    d = got - ref64
    return float(d.pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt()), float(d.abs().max() / ref64.abs().max())


def sharper(got_split, got_f32, ref64, what):
    """The split figures are at most YARD_FACTOR x those of the project's fp32 code on the same inputs + YARD_FLOOR.  Prints and records, then asserts."""
    assert YARD_FACTOR == 3.0 and YARD_FLOOR == 1e-6
    assert torch.isfinite(got_split).all(), f"{what}: non-finite"
    (rs, ms), (rf, mf) = _dist(got_split, ref64), _dist(got_f32, ref64)
    print(f"{what}: split rel rms {rs:.3e} max {ms:.3e} | fp32 rel rms {rf:.3e} max {mf:.3e}")
    record(what, kind="evaluator_split_yardstick", split={"rel_rms": rs, "max": ms}, fp32={"rel_rms": rf, "max": mf}, factor=YARD_FACTOR, floor=YARD_FLOOR)
    assert rs <= YARD_FACTOR * rf + YARD_FLOOR and ms <= YARD_FACTOR * mf + YARD_FLOOR, (what, (rs, ms), (rf, mf))


def test_uniform_split_layer_at_head_size_96_against_float64():
    """D = 192 with 2 heads: the split layer's QKV GEMM writes fp32 rows and the fp32 attention runs on them (the text stack's form)."""
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    D, H, F, T, nseq = 192, 2, 256, 33, 2
    W = random_layer(D, F, 900)
    x0 = EC.rnd(899, nseq, T, D)
    ref64 = EC._encoder_layer({k: v.double() for k, v in W.items()}, "l.", x0.double(), H, None)
    w = {k[2:].replace("self_attn.", ""): v.cuda().contiguous() for k, v in W.items()}
    f32 = ops.encoder_layer_(x0.cuda(), w, H)
    ws = ops.encoder_layer_split_weights(w)
    assert ws["packed"]
    for last in (False, True):
        x, xs = x0.cuda(), ops.split_f32(x0.cuda())
        ops.encoder_layer_split_(x, xs, ws, H, last=last)
        if not last:
            assert torch.equal(bits16(xs), bits16(ops.split_f32(x)))
            first = x
    assert torch.equal(bits32(x), bits32(first))                         # `last` changes the plane write only
    sharper(x, f32, ref64, "split layer, head size 96 (D 192, T 33)")
    # each sequence alone: the same bits (the fp32 attention walks sequences independently)
    a = x0[1:2].cuda()
    ops.encoder_layer_split_(a, ops.split_f32(a), ws, H, last=True)
    assert torch.equal(bits32(a[0]), bits32(x[1]))
    # D = 48: refused by name (and so is F % 32 != 0)
    W48 = random_layer(48, 64, 950)
    w48 = {k[2:].replace("self_attn.", ""): v.cuda().contiguous() for k, v in W48.items()}
    ws48 = ops.encoder_layer_split_weights(w48)
    assert not ws48["packed"]
    y = EC.rnd(951, 1, 5, 48).cuda()
    with pytest.raises(MMDMError, match=r"D % 32 != 0 is not supported \(D=48") as e:
        ops.encoder_layer_split_(y, ops.split_f32(y), ws48, 3)
    assert e.value.status == 4
    so, sl, _, total = seqs((3, 2))
    with pytest.raises(MMDMError, match=r"D % 32 != 0 is not supported \(D=48") as e:
        ops.encoder_layer_ragged_split_(y[0], ops.split_f32(y[0]), ws48, 3, so, sl, 3)
    assert e.value.status == 4


# ---- 4. / 5. the encoders ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["int128", "int256", "ind128"])
def test_split_encode_motion_against_the_reference_and_the_fp32_evaluator(g, case):
    motions, lens = EC.case_motions(g, case)
    batch = lambda: {"motions": motions, "motion_lens": torch.tensor(lens)}
    got = model_of(g, case, "fp32_split").encode_motion(batch())["motion_emb"]
    f32 = model_of(g, case, None).encode_motion(batch())["motion_emb"]
    assert got.shape == (len(lens), 512) and got.is_cuda and not torch.equal(got, f32)
    EC.yardstick(got, g[f"{case}:ref32"], g[f"{case}:ref64"], f"evaluator fp32_split encode_motion {case}")
    sharper(got, f32, g[f"{case}:ref64"], f"evaluator fp32_split encode_motion {case}")
    # precision="fp32" is the default constructor, bit for bit
    assert torch.equal(bits32(model_of(g, case, "fp32").encode_motion(batch())["motion_emb"]), bits32(f32))


def test_split_encode_text_against_the_reference_and_the_fp32_evaluator(g):
    tok = lambda: {"tokens_text": g["text:tokens"]}
    got = model_of(g, "int128", "fp32_split").encode_text(tok())["text_emb"]
    f32 = model_of(g, "int128", None).encode_text(tok())["text_emb"]
    EC.yardstick(got, g["text:ref32"], g["text:ref64"], "evaluator fp32_split encode_text")
    sharper(got, f32, g["text:ref64"], "evaluator fp32_split encode_text")
    assert torch.equal(bits32(model_of(g, "int128", "fp32").encode_text(tok())["text_emb"]), bits32(f32))
    # the token embedding of the split path is the row-kernel build a precision-2 handle runs: a gather and one rounded add, the same bits in both builds
    from mixermdm_amd import ops
    W = EC.case_weights(g, "int128")
    tb, ps = W["token_embedding.weight"].cuda().contiguous(), W["positional_embedding"].cuda().contiguous()
    ids = torch.as_tensor(g["text:tokens"]).to(device="cuda:0", dtype=torch.int32).contiguous()
    assert torch.equal(bits32(ops.token_embed(tb, ids, ps, build=1)), bits32(ops.token_embed(tb, ids, ps)))
    # a prompt's embedding does not depend on the batch
    one = model_of(g, "int128", "fp32_split").encode_text({"tokens_text": g["text:tokens"][1:2]})["text_emb"]
    assert torch.equal(bits32(one[0]), bits32(got[1]))


@pytest.mark.parametrize("case", ["ind128", "ind256"])
def test_split_individual_embeddings_against_the_reference_and_the_fp32_evaluator(gi, case):
    motions, lens = IC.case_motions(gi, case)
    batch = lambda: {"motions": motions, "motion_lens": torch.tensor(lens)}
    got = model_of(gi, case, "fp32_split", "ind").encode_motion_individual(batch())["motion_emb"]
    f32 = model_of(gi, case, None, "ind").encode_motion_individual(batch())["motion_emb"]
    assert got.shape == (8, 512) and got.is_cuda
    ref64 = IC.restated_embeddings(gi, case, torch.float64)
    EC.yardstick(got, gi[f"{case}:motion_ref32"], ref64, f"evaluator fp32_split encode_motion_individual {case}")
    sharper(got, f32, ref64, f"evaluator fp32_split encode_motion_individual {case}")
    assert torch.equal(bits32(model_of(gi, case, "fp32", "ind").encode_motion_individual(batch())["motion_emb"]), bits32(f32))


def test_split_motion_embedding_does_not_depend_on_the_batch(g):
    m = model_of(g, "int128", "fp32_split")
    motions, lens = EC.case_motions(g, "int128")
    enc = lambda mo, ln: m.encode_motion({"motions": mo, "motion_lens": torch.tensor(ln)})["motion_emb"]
    ref = enc(motions, lens)
    for i, n in enumerate(lens):          # alone (in its own, shorter buffer too)
        assert torch.equal(bits32(enc(motions[i:i + 1], [n])[0]), bits32(ref[i])), i
        assert torch.equal(bits32(enc(motions[i:i + 1, :n].contiguous(), [n])[0]), bits32(ref[i])), i
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(bits32(enc(motions[perm], [lens[i] for i in perm])), bits32(ref[perm]))
    poisoned = motions.clone()
    for i, n in enumerate(lens):
        poisoned[i, n:] = float("nan")
    assert torch.equal(bits32(enc(poisoned, lens)), bits32(ref)) and torch.isfinite(ref).all()
    with pytest.raises(ValueError, match="item 1 has motion_lens = 0"):
        enc(motions[:2], [4, 0])


def test_split_individual_embeddings_do_not_depend_on_the_batch(gi):
    m = model_of(gi, "ind128", "fp32_split", "ind")
    motions, lens = IC.case_motions(gi, "ind128")
    enc = lambda mo, ln: m.encode_motion_individual({"motions": mo, "motion_lens": torch.tensor(ln)})["motion_emb"]
    ref = enc(motions, lens)
    assert torch.isfinite(ref).all()
    for i, n in enumerate(lens):
        assert torch.equal(bits32(enc(motions[i:i + 1], [n])), bits32(ref[2 * i:2 * i + 2])), i
    perm = [2, 0, 3, 1]
    assert torch.equal(bits32(enc(motions[perm], [lens[i] for i in perm])), bits32(ref.reshape(4, 2, 512)[perm].reshape(8, 512)))
    # beyond a length only position Y is read (the floor)
    poisoned = motions.clone()
    y = torch.zeros(524, dtype=torch.bool)
    for p in (0, 262):
        y[p + 1:p + 66:3] = True
    for i, n in enumerate(lens):
        poisoned[i, n:, ~y] = float("nan")
    assert torch.equal(bits32(enc(poisoned, lens)), bits32(ref))


# ---- 6. the wrapper and the evaluation pass -------------------------------------------------------------------------------------------------------
def test_split_wrapper_ranks_and_evaluation_pass(g):
    from mixermdm_amd.evaluation import EvaluatorModelWrapper, evaluate_generated
    ws, wf = EvaluatorModelWrapper(model_of(g, "int128", "fp32_split")), EvaluatorModelWrapper(model_of(g, "int128", None))
    assert ws.model.precision == "fp32_split" and wf.model.precision == "fp32"
    motions, lens = EC.case_motions(g, "int128")
    tokens = torch.from_numpy(g["wrap:tokens"])
    names = ["n%d" % i for i in range(5)]
    batch = (names, tokens, motions[..., :262], motions[..., 262:], torch.tensor(lens))
    te, me = ws.get_co_embeddings(batch)
    tf, mf = wf.get_co_embeddings(batch)
    EC.yardstick(te, g["wrap:text_ref32"], g["wrap:text_ref64"], "evaluator fp32_split wrapper text_emb")
    EC.yardstick(me, g["wrap:motion_ref32"], g["wrap:motion_ref64"], "evaluator fp32_split wrapper motion_emb")
    sharper(te, tf, g["wrap:text_ref64"], "evaluator fp32_split wrapper text_emb")
    sharper(me, mf, g["wrap:motion_ref64"], "evaluator fp32_split wrapper motion_emb")
    assert torch.equal(bits32(ws.get_motion_embeddings((names, None, motions[..., :262].numpy(), motions[..., 262:].numpy(), np.array(lens)))), bits32(me))
    generated = [{"motion1": motions[i, :, :262].numpy(), "motion2": motions[i, :, 262:].numpy(), "motion_lens": torch.tensor(lens[i]),
                  "tokens_text": tokens[i]} for i in range(5)]
    mm = [{"mm_motions": motions[:3].reshape(3, 40, 2, 262).numpy(), "motion_lens": torch.tensor(16)}] * 2
    np.random.seed(3)
    res = evaluate_generated(ws, generated, mm_generated=mm, groundtruth=generated[::-1], diversity_times=3, mm_num_times=2)
    # the smallest gap between neighbouring distances is > 100 x the reference's fp32 error: nothing within the yardstick of it can swap two ranks
    assert float(g["wrap:rank_gap"]) > 100 * float(g["wrap:max_err"])
    assert np.array_equal(np.rint(res["r_precision"] * 5).astype(int), g["wrap:top_k"]), (res["r_precision"], g["wrap:top_k"])
    assert set(res) == {"mm_dist", "r_precision", "fid", "diversity", "multimodality"}
    assert all(np.isfinite(np.asarray(v, dtype=float)).all() for v in res.values()), res
    d_got, d_ref = abs(float(res["mm_dist"]) - float(g["wrap:mm_dist64"])), abs(float(g["wrap:mm_dist32"]) - float(g["wrap:mm_dist64"]))
    print(f"fp32_split mm_dist {res['mm_dist']:.9f}: |got - f64| {d_got:.3e}, |ref32 - f64| {d_ref:.3e}")
    record("evaluator fp32_split mm_dist", kind="evaluator_yardstick", got_vs_f64=d_got, ref32_vs_f64=d_ref, factor=YARD_FACTOR, floor=YARD_FLOOR)
    assert d_got <= YARD_FACTOR * d_ref + YARD_FLOOR
    assert abs(res["fid"]) < 1e-6 and res["diversity"] > 0 and res["multimodality"] > 0          # the same set as its own ground truth
