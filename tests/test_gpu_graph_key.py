"""GPU: the key of the step-graph cache (csrc/mmdm.hip GraphKey) in one place.  A captured step graph bakes in nine things; a call that differs from
an earlier one in ONE of them must capture a graph of its own, and a call that differs in none must replay.  A field that is stored but not compared
gives no error -- it replays another call's kernels -- so every field is walked here, one at a time.

The key of a call, by mmdm_begin's rules (begin_impl): a uniform call is (B, T, S, 0, masked, 0, 0, noise, pinned); a ragged call is
(B, tiles(max len), S, rows, 0, trows, tT, noise, pinned) with tiles(t) = (t + 63) // 64, rows = sum(lens) rounded up to the 128-row bucket, and -- with MDM
as denoiser 1 only -- trows = sum(lens) + B rounded up likewise, tT = tiles(max len + 1); trows = tT = 0 otherwise.

Two-chain handle (tests/test_gpu_ragged.py small(): latent 128, ff 256, 2 layers, 2 heads, max_batch 8, ddim20; max_frames 128, not 64, because the
query-tile pair needs an item of 65 frames).  Every call, its key, and the earlier call it differs from in exactly one field:
    base      B 1, T 24                    (1, 24, 20,   0, 0, 0, 0, 0, 0)   the first call
    B         B 2, T 24                    (2, 24, 20,   0, 0, 0, 0, 0, 0)   base: B
    T         B 1, T 40                    (1, 40, 20,   0, 0, 0, 0, 0, 0)   base: T
    S         ddim50                       (1, 24, 50,   0, 0, 0, 0, 0, 0)   base: S
    masked    key mask [1, 24] set         (1, 24, 20,   0, 1, 0, 0, 0, 0)   base: masked      (cleared again afterwards)
    buffer    eta 1, noise buffer          (1, 24, 20,   0, 0, 0, 0, 1, 0)   base: noise
    seed      eta 1, device generator      (1, 24, 20,   0, 0, 0, 0, 2, 0)   buffer: noise
    pinned    x_start given                (1, 24, 20,   0, 0, 0, 0, 0, 1)   base: pinned
    B2T1      B 2, T 1                     (2,  1, 20,   0, 0, 0, 0, 0, 0)   B: T              (the uniform call next to the first ragged one)
    r40_17    lens (40, 17):  57 rows      (2,  1, 20, 128, 0, 0, 0, 0, 0)   B2T1: rows
    r64_1     lens (64, 1):   65 rows      (2,  1, 20, 128, 0, 0, 0, 0, 0)   THE SAME KEY as r40_17: replays, no capture -- 64 frames are one query tile
    r65_1     lens (65, 1):   66 rows      (2,  2, 20, 128, 0, 0, 0, 0, 0)   r64_1: T (query tiles 1 -> 2)
    r40_17_1  lens (40, 17, 1):  58 rows   (3,  1, 20, 128, 0, 0, 0, 0, 0)   r40_17: B
    r64_64_40 lens (64, 64, 40): 168 rows  (3,  1, 20, 256, 0, 0, 0, 0, 0)   r40_17_1: rows (128 -> 256)
(the stride pair (40, 17) / (64, 64, 40) differs in B as well, hence r40_17_1 between them; (64, 1) cannot capture beside (40, 17), so it is held as a replay.)

MDM handle (tests/test_gpu_ragged_mdm.py small(): MDM as denoiser 1, max_frames 64, ddim20); 64 frames are one tile of frames and two of tokens:
    m63       lens (63,):     63 rows,  64 token rows   (1, 1, 20, 128, 0, 128, 1, 0, 0)   the first call
    m64       lens (64,):     64 rows,  65 token rows   (1, 1, 20, 128, 0, 128, 2, 0, 0)   m63: tT (token tiles 1 -> 2)
    m64_62    lens (64, 62): 126 rows, 128 token rows   (2, 1, 20, 128, 0, 128, 2, 0, 0)   m64: B
    m64_63    lens (64, 63): 127 rows, 129 token rows   (2, 1, 20, 128, 0, 256, 2, 0, 0)   m64_62: trows (token stride 128 -> 256)

The whole sequence runs twice with use_graph=True, two steps per call: the first pass captures once per new key, the second captures nothing, and the
replay count grows by two per call throughout.  MMDM_GRAPH_CACHE = 32 keeps every graph cached."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("B", "T", "S", "rows", "masked", "trows", "tT", "noise", "pinned")
BUCKET = 128


def tiles(t):
    return (t + 63) // 64


def bucket(n):
    return (n + BUCKET - 1) // BUCKET * BUCKET


def key(B=None, T=None, lens=None, S=20, masked=0, noise=0, pinned=0, mdm=False):
    """The graph key of a call, computed by hand from begin_impl's rules."""
    if lens is None:
        return (B, T, S, 0, masked, 0, 0, noise, pinned)
    B, mx, total = len(lens), max(lens), sum(lens)
    return (B, tiles(mx), S, bucket(total), masked, bucket(total + B) if mdm else 0, tiles(mx + 1) if mdm else 0, noise, pinned)


# (name, call keywords, the earlier call it stands next to, the ONE field it differs in -- None: the same key, a replay)
TWO_CHAIN = [
    ("base", dict(B=1, T=24), None, None),
    ("B", dict(B=2, T=24), "base", "B"),
    ("T", dict(B=1, T=40), "base", "T"),
    ("S", dict(B=1, T=24, S=50), "base", "S"),
    ("masked", dict(B=1, T=24, masked=1), "base", "masked"),
    ("buffer", dict(B=1, T=24, noise=1), "base", "noise"),
    ("seed", dict(B=1, T=24, noise=2), "buffer", "noise"),
    ("pinned", dict(B=1, T=24, pinned=1), "base", "pinned"),
    ("B2T1", dict(B=2, T=1), "B", "T"),
    ("r40_17", dict(lens=(40, 17)), "B2T1", "rows"),
    ("r64_1", dict(lens=(64, 1)), "r40_17", None),
    ("r65_1", dict(lens=(65, 1)), "r64_1", "T"),
    ("r40_17_1", dict(lens=(40, 17, 1)), "r40_17", "B"),
    ("r64_64_40", dict(lens=(64, 64, 40)), "r40_17_1", "rows"),
]
MDM = [
    ("m63", dict(lens=(63,)), None, None),
    ("m64", dict(lens=(64,)), "m63", "tT"),
    ("m64_62", dict(lens=(64, 62)), "m64", "B"),
    ("m64_63", dict(lens=(64, 63)), "m64_62", "trows"),
]


def expected_captures(seq, mdm):
    """Checks on the host that every call differs from the earlier call named beside it in exactly the intended field, and returns, per call, whether
    its key is new (1: it must capture) or was seen before (0: it must replay)."""
    keys, seen, new = {}, set(), []
    for name, kw, prev, field in seq:
        k = key(mdm=mdm, **kw)
        keys[name] = k
        if prev is not None:
            diff = [f for f, a, b in zip(FIELDS, keys[prev], k) if a != b]
            assert diff == ([field] if field else []), (name, prev, diff, keys[prev], k)
        new.append(0 if k in seen else 1)
        seen.add(k)
    return new


def call(s, cw, B=None, T=None, lens=None, S=20, masked=0, noise=0, pinned=0, seed=0):
    """One two-step call with use_graph=True; the handle is left as it was found (ddim20, eta 0, no mask)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    if S != 20:
        s.set_schedule("ddim%d" % S)
    if lens is not None:
        s.begin_ragged(rnd(len(lens), cw), [rnd(t, 524) for t in lens], lens)
    else:
        kw = {}
        if masked:
            valid = torch.ones(B, T, dtype=torch.bool)
            valid[:, T - 4:] = False
            s.set_key_mask(valid)
        if noise:
            s.set_eta(1.0)
            kw.update(noise=rnd(S, B, T, 524)) if noise == 1 else kw.update(seed=1234)
        if pinned:
            kw.update(x_start=rnd(B, T, 524))
        s.begin(rnd(B, cw), rnd(B, T, 524), **kw)
    s.run(2, use_graph=True)
    s.synchronize()
    if masked:
        s.set_key_mask(None)
    if noise:
        s.set_eta(0.0)
    if S != 20:
        s.set_schedule("ddim20")


def walk(s, cw, seq, mdm):
    new = expected_captures(seq, mdm)
    cap0, rep0, _ = s.graph_stats()
    assert (cap0, rep0) == (0, 0)
    calls = 0
    for rnd_ in range(2):
        for (name, kw, _, _), fresh in zip(seq, new):
            cap, rep, _ = s.graph_stats()
            call(s, cw, seed=calls, **kw)
            calls += 1
            cap2, rep2, cached = s.graph_stats()
            want = fresh if rnd_ == 0 else 0
            assert cap2 - cap == want, (rnd_, name, "captures", cap, cap2, "expected", want)
            assert rep2 - rep == 2, (rnd_, name, "replays", rep, rep2)
    assert s.graph_stats() == (sum(new), 2 * calls, sum(new))       # nothing was evicted


def test_every_key_field_alone_separates_two_captured_graphs(monkeypatch):
    monkeypatch.setenv("MMDM_GRAPH_CACHE", "32")
    from test_gpu_ragged import small
    s = small(max_batch=8, max_frames=128)
    try:
        s.set_schedule("ddim20")
        walk(s, 8 * 768, TWO_CHAIN, mdm=False)
    finally:
        s.close()


def test_token_stride_and_token_tiles_separate_graphs_with_mdm_as_denoiser_1(monkeypatch):
    monkeypatch.setenv("MMDM_GRAPH_CACHE", "32")
    from test_gpu_ragged_mdm import small
    s = small()
    try:
        walk(s, 6 * 768 + 2 * 128, MDM, mdm=True)
    finally:
        s.close()
