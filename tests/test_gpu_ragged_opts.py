"""GPU: the loop's options -- eta > 0 (noise buffer or device generator), init_image / skip_timesteps, x_start -- on RAGGED batches
(mmdm_begin_ragged_opts, Sampler.begin_ragged's keywords, MixerMDM.sample_many's eta / skip_timesteps).  The rule of ragged batches holds with
every option: each item of a ragged batch is BITWISE the same item sampled alone with the same options.  Parity with the reference is inherited
through that identity (the uniform option calls are pinned by tests/golden/sampler_opts.npz; the reference has no ragged batch to capture), so
every comparison here is exact and no tolerance appears.  Small handles of tests/test_gpu_ragged.py (D = 128, head size 64, max_frames 64), ddim4."""
import ctypes as C
import pytest
import torch

from test_gpu_ragged import small, inputs, LENS, EDGE_LENS

pytestmark = pytest.mark.gpu

S = 4                                     # ddim4
SEEDS = (0x1234_5678_9ABC_DEF1, 7, (1 << 63) + 5, 0xFFFF_FFFF_0000_0001, 99)      # high key words, both key words, a small one
CASES = ("pin", "init", "skip", "eta_buf", "eta_seed", "all")
PERM = [3, 0, 4, 2, 1]


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


class Batch:
    """One set of items with everything an option can take, per item: x_start (a few frames longer than the item: cut to T_i), init_image (scaled by 0.5
    as the uniform tests do), a noise buffer and a seed."""

    def __init__(self, lens, seed=0, cw=8 * 768):
        self.lens = tuple(lens)
        self.cond, self.xs = inputs(lens, cw=cw, seed=seed)
        self.x_start = [rnd(1000 + seed + b, t + 3, 524) for b, t in enumerate(lens)]
        self.init = [0.5 * rnd(2000 + seed + b, t, 524) for b, t in enumerate(lens)]
        self.noise = [rnd(3000 + seed + b, S, t, 524) for b, t in enumerate(lens)]
        self.seeds = [SEEDS[b % len(SEEDS)] + b // len(SEEDS) for b in range(len(lens))]

    def kwargs(self, case, items=None):
        """(keywords of the ragged call over `items`, keywords of item b's stand-alone call)."""
        idx = list(range(len(self.lens))) if items is None else list(items)
        eta = {"eta_buf": 0.5, "eta_seed": 1.0, "all": 1.0}.get(case, 0.0)
        skip = {"skip": 2, "all": 1}.get(case, 0)
        rag, one = dict(eta=eta, skip_timesteps=skip), lambda b: dict(eta=eta, skip_timesteps=skip)
        parts = [one]
        if case in ("pin", "all"):
            rag["x_start"] = [self.x_start[b] for b in idx]
            parts.append(lambda b: dict(x_start=self.x_start[b][None]))
        if case in ("init", "all"):
            rag["init_image"] = [self.init[b] for b in idx]
            parts.append(lambda b: dict(init_image=self.init[b][None]))
        if case == "eta_buf":
            rag["noise"] = [self.noise[b] for b in idx]
            parts.append(lambda b: dict(noise=self.noise[b][:, None]))
        if case in ("eta_seed", "all"):
            rag["seeds"] = [self.seeds[b] for b in idx]
            parts.append(lambda b: dict(seed=self.seeds[b]))
        return rag, lambda b: {k: v for p in parts for k, v in p(b).items()}

    def alone(self, s, case, use_graph=False):
        _, one = self.kwargs(case)
        out = [s.sample(self.cond[b:b + 1], x[None], use_graph=use_graph, **one(b))[0] for b, x in enumerate(self.xs)]
        s.set_eta(0.0)
        return out

    def ragged(self, s, case, use_graph, items=None):
        idx = list(range(len(self.lens))) if items is None else list(items)
        rag, _ = self.kwargs(case, idx)
        out = s.sample_ragged(self.cond[idx], [self.xs[b] for b in idx], [self.lens[b] for b in idx], use_graph=use_graph, **rag)
        s.set_eta(0.0)
        return out


def same(items, ref, what=""):
    assert len(items) == len(ref)
    for b, (it, r) in enumerate(zip(items, ref)):
        assert it.shape == r.shape and torch.isfinite(it).all(), (what, b)
        assert torch.equal(it, r), (what, b, tuple(r.shape), (it - r).abs().max().item())


class Shared:
    """The fp32 handle several tests share, the stand-alone references of every case and the plain ragged result (computed once, never modified)."""

    def __init__(self):
        self.s, self.bt, self.ref, self.plain = None, Batch(LENS, seed=1), {}, None

    def handle(self):
        if self.s is None:
            self.s = small()
            self.s.set_schedule("ddim4")
        if self.plain is None:
            self.plain = self.s.sample_ragged(self.bt.cond, self.bt.xs, LENS, use_graph=False)
        return self.s

    def alone(self, case):
        if case not in self.ref:
            self.ref[case] = self.bt.alone(self.handle(), case)
        return self.ref[case]

    def close(self):
        if self.s is not None:
            self.s.close()
            self.s = None


@pytest.fixture(scope="module")
def shared():
    sh = Shared()
    yield sh
    sh.close()


@pytest.fixture
def fp32(shared):
    s = shared.handle()
    return s, shared.bt, shared.plain, shared.alone


@pytest.fixture
def own_handle(shared):
    """For a test that creates AND closes a handle with captured graphs of its own: the shared handle is closed first (and made again by the next test
    that wants it).  In this runtime, destroying a graph exec while another handle's execs are alive makes that handle's next hipGraphLaunch crash
    (csrc/mmdm.hip, retire_exec) -- so no handle of this file outlives the destruction of another one's graphs."""
    shared.close()


# ---------------------------------------------------------------------------------------------------
# 1. items equal their stand-alone calls, bitwise
# ---------------------------------------------------------------------------------------------------
def check_case(s, bt, case, ref, plain):
    """LENS = (40, 17, 64, 1, 33): 155 frames in a 256-row group -- padding rows, a noise slot stride != rows, T = 1."""
    eager = bt.ragged(s, case, use_graph=False)
    assert s.rows == 256 and sum(bt.lens) == 155
    same(eager, ref, case + " eager")
    same(bt.ragged(s, case, use_graph=True), ref, case + " graph")
    same(bt.ragged(s, case, use_graph=True, items=PERM), [ref[i] for i in PERM], case + " permuted")
    if plain is not None:                                   # and it is not the plain loop (the uniform test's bar)
        real = torch.cat([(a - b).abs().flatten() for a, b in zip(eager, plain)])
        print("%s: mean |case - plain| over the real frames %.3f" % (case, float(real.mean())))
        assert float(real.mean()) > 0.05, (case, float(real.mean()))


@pytest.mark.parametrize("case", CASES)
def test_ragged_option_items_equal_their_stand_alone_calls(fp32, case):
    s, bt, plain, alone = fp32
    check_case(s, bt, case, alone(case), plain)
    same(s.sample_ragged(bt.cond, bt.xs, LENS, use_graph=True), plain, "plain afterwards")


@pytest.mark.parametrize("precision", ["fp32_split", "bf16", "bf16_fp8"])
def test_all_options_in_every_precision_mode(own_handle, precision):
    s = small(precision=precision)
    s.set_schedule("ddim4")
    bt = Batch(LENS, seed=1)
    plain = s.sample_ragged(bt.cond, bt.xs, LENS, use_graph=False)
    check_case(s, bt, "all", bt.alone(s, "all"), plain)
    s.close()


# ---------------------------------------------------------------------------------------------------
# 2. one seed, equal lengths: the ragged batch is the uniform call
# ---------------------------------------------------------------------------------------------------
def test_one_seed_and_equal_lengths_is_the_uniform_call(fp32):
    from mixermdm_amd import ops
    s = fp32[0]
    SEED = SEEDS[0]
    lens = (20, 20, 20)
    cond, xs = inputs(lens, seed=21)
    uni = s.sample(cond, torch.stack(xs), use_graph=False, eta=1.0, seed=SEED)
    for use_graph in (False, True):
        same(s.sample_ragged(cond, xs, lens, use_graph=use_graph, eta=1.0, seeds=SEED), list(uni), "one seed")
    # the seed form is the buffer form filled by ops.randn at (seed_b, row_b) -- here with rows and seeds of a mixed batch
    lens2, seeds, rows = (20, 9, 33), [SEED, SEED, 5], [0, 2, 1]
    cond2, xs2 = inputs(lens2, seed=22)
    a = s.sample_ragged(cond2, xs2, lens2, use_graph=False, eta=1.0, seeds=seeds, noise_rows=rows)
    buf = [torch.stack([ops.randn(sd, k, r + 1, t)[r] for k in range(S)]) for sd, r, t in zip(seeds, rows, lens2)]
    b = s.sample_ragged(cond2, xs2, lens2, use_graph=False, eta=1.0, noise=buf)
    same(a, b, "seed form vs buffer form")
    c = s.sample_ragged(cond2, xs2, lens2, use_graph=False, eta=1.0, seeds=seeds, noise_rows=[0, 1, 1])
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and not torch.equal(c[1], a[1])      # an item's row counts, and only for that item
    s.set_eta(0.0)


# ---------------------------------------------------------------------------------------------------
# 3. graphs
# ---------------------------------------------------------------------------------------------------
def test_graphs_of_ragged_option_calls(own_handle):
    """a and b: the same bucket (256 rows), the same B, one query tile -- and 155 vs 204 frames, so another slot stride of the packed noise buffer.  In the
    order a, b, a under replay they take ONE capture, and each equals its eager run: a stride baked into the captured node fails on b."""
    from mixermdm_amd._lib import BeginRaggedOptions, check
    s = small()
    s.set_schedule("ddim4")
    A, Bb = Batch((40, 17, 64, 1, 33), seed=31), Batch((64, 60, 10, 50, 20), seed=32)
    plain = s.sample_ragged(A.cond, A.xs, A.lens, use_graph=True)
    cap0 = s.graph_stats()[0]
    assert cap0 == 1
    eager = {id(bt): bt.ragged(s, "eta_buf", use_graph=False) for bt in (A, Bb)}
    for bt in (A, Bb, A):
        same(bt.ragged(s, "eta_buf", use_graph=True), eager[id(bt)], "buffer form a, b, a")
        assert s.rows == 256
    assert s.graph_stats()[0] == cap0 + 1                              # one capture for the three
    # new option values replay the same graph
    kw = dict(eta=0.7, noise=[rnd(4000 + b, S, t, 524) for b, t in enumerate(A.lens)])
    g2 = s.sample_ragged(A.cond, A.xs, A.lens, use_graph=True, **kw)
    assert s.graph_stats()[0] == cap0 + 1
    same(g2, s.sample_ragged(A.cond, A.xs, A.lens, use_graph=False, **kw), "new values")
    assert not torch.equal(g2[0], eager[id(A)][0])
    # the pinned buffer form, the seed form and the un-pinned seed form are other entries
    pin = dict(eta=0.5, noise=A.noise, x_start=A.x_start)
    gp = s.sample_ragged(A.cond, A.xs, A.lens, use_graph=True, **pin)
    assert s.graph_stats()[0] == cap0 + 2
    same(gp, s.sample_ragged(A.cond, A.xs, A.lens, use_graph=False, **pin), "pinned buffer form")
    same(A.ragged(s, "all", use_graph=True), A.ragged(s, "all", use_graph=False), "all")
    assert s.graph_stats()[0] == cap0 + 3
    same(A.ragged(s, "eta_seed", use_graph=True), A.ragged(s, "eta_seed", use_graph=False), "seed form")
    assert s.graph_stats()[0] == cap0 + 4
    same(Bb.ragged(s, "eta_seed", use_graph=True), Bb.ragged(s, "eta_seed", use_graph=False), "seed form, other lengths")
    assert s.graph_stats()[0] == cap0 + 4
    # the plain ragged call is what it was, on its old graph; a zeroed options struct is mmdm_begin_ragged
    same(s.sample_ragged(A.cond, A.xs, A.lens, use_graph=True), plain, "plain afterwards")
    assert s.graph_stats()[0] == cap0 + 4
    cond, x = A.cond.cuda(), torch.cat(A.xs).cuda()
    arr = (C.c_int * len(A.lens))(*A.lens)
    for o in (C.byref(BeginRaggedOptions()), None):
        with torch.cuda.device(s.device):
            check(s.lib.mmdm_begin_ragged_opts(s.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x.data_ptr()), len(A.lens), arr, o, s._s()), s.h)
            check(s.lib.mmdm_run(s.h, S, 1, s._s()), s.h)
        s.stream.synchronize()
        got = s.state()["pred_xstart2"]
        same([got[o_:o_ + t] for o_, t in s.item_slices()], plain, "zeroed struct")
    assert s.graph_stats()[0] == cap0 + 4
    s.close()


# ---------------------------------------------------------------------------------------------------
# 4. tile edges
# ---------------------------------------------------------------------------------------------------
def test_all_options_at_the_tile_edges(own_handle):
    s = small(max_batch=10, max_frames=64)
    s.set_schedule("ddim4")
    bt = Batch(EDGE_LENS, seed=41)
    ref = bt.alone(s, "all")
    same(bt.ragged(s, "all", use_graph=True), ref, "edges")
    assert s.rows >= sum(EDGE_LENS)
    s.close()


# ---------------------------------------------------------------------------------------------------
# 5. MDM as MODEL1
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp32_split"])
def test_all_options_with_mdm_as_model1(own_handle, precision):
    """The small MDM configuration of tests/test_gpu_ragged_mdm.py (D1 = 128, two heads of 64, two layers)."""
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict, synthetic_stats
    from test_gpu_ragged_mdm import DIMS
    sd = synthetic_state_dict(seed=7, std=0.05, bias_std=0.02, mixing_mode=4, model1="MDM", single_only=False, d1_latent=128, d1_ff=256, d1_layers=2, **DIMS)
    s = Sampler(d_heads=2, m_heads=2, max_batch=8, max_frames=64, mixing_mode=4, model1_kind=1, d1_latent=128, d1_ff=256, d1_layers=2, d1_heads=2,
                precision=precision, **DIMS)
    s.load_state_dict(sd)
    st = synthetic_stats()
    s.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
    s.prepare()
    s.set_schedule("ddim4")
    bt = Batch(LENS, seed=51, cw=6 * 768 + 2 * 128)
    ref = bt.alone(s, "all")
    same(bt.ragged(s, "all", use_graph=True), ref, "MDM all")
    same(bt.ragged(s, "all", use_graph=False, items=PERM), [ref[i] for i in PERM], "MDM all, permuted, eager")
    s.close()


# ---------------------------------------------------------------------------------------------------
# 6. refusals, each by its message and status
# ---------------------------------------------------------------------------------------------------
def test_refusals(fp32):
    from mixermdm_amd._lib import MMDMError, BeginRaggedOptions, check
    s, bt, plain, _ = fp32
    ARG, STATE, UNSUPPORTED = 1, 2, 4            # mmdm_status (include/mmdm.h)

    def refused(match, fn, status):
        with pytest.raises(MMDMError, match=match) as e:
            fn()
        assert e.value.status == status

    begin = lambda **kw: s.begin_ragged(bt.cond, bt.xs, LENS, **kw)
    s.set_eta(0.5)
    refused("mmdm_begin_ragged_opts: eta is set on the handle and the call names no noise source", lambda: begin(x_start=bt.x_start), STATE)
    refused("mmdm_begin_ragged_opts: eta is set on the handle and the call names no noise source", lambda: begin(skip_timesteps=1), STATE)
    # the option-less call keeps its entry point, status and sentence, which now goes on to say where ragged noise comes from
    refused(r"mmdm_begin_ragged: eta is set on the handle; the stochastic update covers uniform batches and ragged calls that name a noise source "
            r"\(mmdm_begin_ragged_opts\)", lambda: begin(), UNSUPPORTED)
    refused("the noise buffer holds 3 steps, 4 are left", lambda: begin(noise=[n[:3] for n in bt.noise]), ARG)
    begin(noise=[n[:3] for n in bt.noise], skip_timesteps=1)                     # 3 slots are enough for 3 steps ...
    s.seek(1)
    refused("run past the call's noise buffer", lambda: s.run(2), ARG)         # ... and loop positions 2, 3 are not among them
    refused(r"skip_timesteps=4 outside \[0, 4\)", lambda: begin(seeds=1, skip_timesteps=S), ARG)
    refused(r"skip_timesteps=-1 outside \[0, 4\)", lambda: begin(seeds=1, skip_timesteps=-1), ARG)
    # source 2 without item_seed: only the C ABI can say that
    cond, x = bt.cond.cuda(), torch.cat(bt.xs).cuda()
    arr = (C.c_int * len(LENS))(*LENS)
    o = BeginRaggedOptions()
    o.noise_source = 2
    with torch.cuda.device(s.device):
        refused("noise_source 2 needs item_seed", lambda: check(s.lib.mmdm_begin_ragged_opts(s.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x.data_ptr()), len(LENS), arr,
                                                                                               C.byref(o), s._s()), s.h), ARG)
    s.set_eta(0.0)
    refused("mmdm_begin_ragged_opts: a noise source is given and no eta table is set", lambda: begin(seeds=list(bt.seeds)), STATE)
    refused("mmdm_begin_ragged_opts: a noise source is given and no eta table is set", lambda: begin(noise=bt.noise), STATE)
    # a key mask on a ragged call stays refused
    s.set_key_mask(torch.ones(len(LENS), 64, dtype=torch.bool))
    refused("a key mask is set on the handle; ragged batches carry their lengths instead", lambda: begin(x_start=bt.x_start), UNSUPPORTED)
    s.set_key_mask(None)
    # the Sampler's own errors
    with pytest.raises(ValueError, match="not both"):
        begin(noise=bt.noise, seeds=1)
    with pytest.raises(ValueError, match="need seeds"):
        begin(noise_rows=[0] * len(LENS))
    with pytest.raises(ValueError, match="x_start of item 0"):
        begin(x_start=[t[:5] for t in bt.x_start])
    with pytest.raises(ValueError, match="init_image"):
        begin(init_image=bt.x_start)
    with pytest.raises(ValueError, match="4 seeds for 5 items"):
        begin(seeds=[1, 2, 3, 4])
    same(s.sample_ragged(bt.cond, bt.xs, LENS, use_graph=False), plain, "the handle is as it was")
    # the single-person sampler takes ragged batches and none of the options (eager: this handle is closed beside the shared one and must own no graph)
    k = small(single_only=True)
    k.set_schedule("ddim4")
    c1, x1 = inputs(LENS, width=262, cw=768, seed=5)
    ref = k.sample_ragged(c1, x1, LENS, use_graph=False)
    refused("mmdm_begin_ragged_opts: step noise, x_start, init_image and skip_timesteps cover the two-chain MixerMDM sampler",
            lambda: k.begin_ragged(c1, x1, LENS, skip_timesteps=1), UNSUPPORTED)
    refused("cover the two-chain MixerMDM sampler", lambda: k.begin_ragged(c1, x1, LENS, seeds=1), UNSUPPORTED)
    same(k.sample_ragged(c1, x1, LENS, use_graph=False), ref, "single-person sampler afterwards")
    k.close()


# ---------------------------------------------------------------------------------------------------
# 7. the facade
# ---------------------------------------------------------------------------------------------------
def test_sample_many_takes_the_options(own_handle):
    import os
    from mixermdm_amd.configs import get_config
    from mixermdm_amd.models import MixerMDM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = MixerMDM(get_config(os.path.join(root, "configs", "models", "MixerMDM.yaml")), sampling_strategy="ddim4", config_root=root)
    m.init_synthetic(seed=0)
    m = m.to("cuda:0")
    m.eval()
    lens, reps = (33, 17, 40), (1, 2, 1)

    def batches(named=True):
        out = []
        for i, (t, r) in enumerate(zip(lens, reps)):
            g = torch.Generator().manual_seed(60 + i)
            b = {"cond": torch.randn(r, 8 * 768, generator=g).cuda(), "x_T": torch.randn(r, t, 524, generator=g).cuda(), "motion_lens": torch.tensor([t]),
                 "text": ["x"] * r, "x_start": torch.randn(r, t + 2, 524, generator=g).cuda(), "init_image": (0.5 * torch.randn(r, t, 524, generator=g)).cuda()}
            if named:
                b["seed"] = 500 + i
            out.append(b)
        return out

    def equal(got, ref, what):
        for g, r, t, nb in zip(got, ref, lens, reps):
            assert g["output"].shape == (nb, t, 524) and torch.equal(g["output"], r["output"]), (what, t)
            assert set(g) == set(r)
            for k in r:
                if k != "output":
                    assert len(g[k]) == len(r[k]) == 3, (what, k, len(g[k]), len(r[k]))          # S - skip entries
                    for a, b in zip(g[k], r[k]):
                        assert a.shape == b.shape and torch.equal(a, b), (what, k, t)

    plain = m.sample_many([{k: v for k, v in b.items() if k in ("cond", "x_T", "motion_lens", "text")} for b in batches()], batching="ragged")
    for mode in ("eval_intermediate", "eval"):
        seq = m.sample_many(batches(), mode=mode, batching="sequential", eta=1.0, skip_timesteps=1)
        rag = m.sample_many(batches(), mode=mode, batching="ragged", eta=1.0, skip_timesteps=1)
        equal(rag, seq, mode)
    assert float((rag[0]["output"] - plain[0]["output"]).abs().mean()) > 0.05
    # the two-motion batch: motion j is (seed, row j) -- the two differ, and motion 1 alone under the same seed is row 0, another motion
    two = batches()[1]
    assert not torch.equal(rag[1]["output"][0], rag[1]["output"][1])
    solo = {k: (v[1:] if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in two.items()}
    solo["text"] = ["x"]
    got = m.sample_many([solo], batching="ragged", eta=1.0, skip_timesteps=1)[0]["output"][0]
    assert not torch.equal(got, rag[1]["output"][1])
    smp = m._sampler
    ref = smp.sample_ragged(two["cond"][1:], [two["x_T"][1]], [17], eta=1.0, skip_timesteps=1, seeds=[501], noise_rows=[1], x_start=[two["x_start"][1]],
                            init_image=[two["init_image"][1]])
    smp.set_eta(0.0)
    assert torch.equal(ref[0], rag[1]["output"][1])
    # the noise buffer form
    bn = batches(named=False)
    for i, b in enumerate(bn):
        b["step_noise"] = rnd(70 + i, 3, b["x_T"].shape[0], b["x_T"].shape[1], 524).cuda()
    equal(m.sample_many([dict(b) for b in bn], batching="ragged", eta=0.5, skip_timesteps=1),
          m.sample_many([dict(b) for b in bn], batching="sequential", eta=0.5, skip_timesteps=1), "step_noise")
    # an un-named seed comes from torch's default generator, one per batch in batch order
    torch.manual_seed(5)
    a = m.sample_many(batches(named=False), batching="ragged", eta=1.0, skip_timesteps=1)
    torch.manual_seed(5)
    b = m.sample_many(batches(named=False), batching="sequential", eta=1.0, skip_timesteps=1)
    c = m.sample_many(batches(named=False), batching="ragged", eta=1.0, skip_timesteps=1)
    equal(a, b, "un-named seeds")
    assert not torch.equal(a[0]["output"], c[0]["output"])
    # one noise form, x_start / init_image for all or none, no options in flight
    mixed = batches()
    del mixed[1]["seed"]
    mixed[1]["step_noise"] = bn[1]["step_noise"]
    with pytest.raises(ValueError, match="batch 1 .*one noise form per call"):
        m.sample_many(mixed, batching="ragged", eta=1.0, skip_timesteps=1)
    some = batches()
    del some[2]["x_start"]
    with pytest.raises(ValueError, match="batch 2 .*'x_start'"):
        m.sample_many(some, batching="ragged", eta=1.0)
    with pytest.raises(ValueError, match="inflight"):
        m.sample_many(batches(), batching="inflight", eta=1.0)
    with pytest.raises(ValueError, match="inflight"):
        m.sample_many(batches(), batching="inflight")                      # x_start / init_image in the dicts
    # the handle is left at eta = 0: a plain sample_many is bitwise what it was
    again = m.sample_many([{k: v for k, v in b.items() if k in ("cond", "x_T", "motion_lens", "text")} for b in batches()], batching="ragged")
    for g, r in zip(again, plain):
        assert torch.equal(g["output"], r["output"])
        assert len(g["influence_i1"]) == 4 and all(torch.equal(x, y) for x, y in zip(g["influence_i1"], r["influence_i1"]))
    m._sampler.close()
