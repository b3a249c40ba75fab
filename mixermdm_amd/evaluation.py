"""The InterCLIP evaluator on the GPU: motion encoder on ragged batches, text encoder, the evaluation wrapper and the metric functions.

Reference: MotionEncoder / InterCLIP  src/evaluation/models.py;  EvaluatorModelWrapper / build_models  src/evaluation/utils.py:107-235;
the metric functions  src/utils/metrics.py;  evaluate_matching_score / evaluate_fid / evaluate_diversity / evaluate_multimodality
src/scripts/eval/mixermdm.py:17-114.

The reference pads every motion of a batch to the longest, prepends a query token, runs a post-norm ``nn.TransformerEncoder`` with a prefix
key-padding mask and keeps the token's row.  A padded query row never reaches a valid key's output, so nothing is lost by not computing it:
here every item is a token sequence of ``1 + min(T, motion_lens[i])`` rows, the sequences lie back to back, and the encoder is the library's
ragged post-norm layer (``ops.encoder_layer_ragged_``).  All arithmetic of the two encoders runs in the HIP library, fp32; Python orders the
calls (the pattern of ``text.py``: a host composition of ops, no handle).  The metrics are float64 numpy / scipy on the host: the matrices
are 32 x 32 and 512 x 512.

Order convention (the reference's docstring: "the results does not following the order of inputs"): ``get_co_embeddings`` returns both
embeddings in the order ``np.argsort(motion_lens.tolist())[::-1]`` -- longest motion first, computed with numpy on the host exactly so.

The individual half of the reference's table (EvaluatorModelWrapperIndividual  src/evaluation/utils.py:237-383; calculate_f_score
src/scripts/eval/mixermdm.py:117-121, 216-241): every person of an interaction is centred on its own and encoded by an InterCLIP in MODE: individual
-- ``InterCLIP.encode_motion_individual`` over the fused centre-and-pack kernel (``ops.center_pack``), 2B embeddings in the order p1 of item 0, p2 of
item 0, ..., no length sort -- and ``summarize_replications`` / ``f_score_summary`` give the mean, the confidence interval and the harmonic mean.

Bitwise: an item's motion embedding does not depend on the batch it is encoded in, on its position in it, or on what the buffer holds beyond
its length (the reference's own batched result differs from its alone result in the last bits).

Precision: ``InterCLIP(cfg, precision="fp32_split")`` runs both encoders on the fp16 matrix cores at fp32 accuracy (DESIGN section 7's operand format): the
weight matrices get fp16-plane twins once in ``load_state_dict``, the pack kernels write the embedding operand as planes, ``motion_tokens_split_`` writes
layer 0's rows and planes, the layers are the library's split post-norm layer (ragged for motions; the text stack's 96-wide heads take its fp32 attention),
and LayerNorm / Linear / normalise close the path in the row-kernel build a precision-2 sampler handle uses.  ``precision="fp32"`` (the default) is the path
above, unchanged.  The bitwise statement holds in both modes.
"""
import numpy as np
import torch

from . import ops
from .sampler import pe_table
from .text import _ENC_KEYS, _eot_rows, tokenize

NFEATS = 262          # pose features per person as generated; the encoder drops the last 4 of every person (models.py:60-62)
EMB_DIM = 512
TEXT_DIM, TEXT_HEADS, TEXT_LAYERS = 768, 8, 8          # models.py:111-122
PE_KEY = "motion_encoder.sequence_pos_encoder.pe"
emb_scale = 6         # metrics.py:8
PRECISIONS = ("fp32", "fp32_split")


def embed_k_pad(npers, precision="fp32"):
    """Columns of the embedding GEMM's A operand (and of the zero-padded embed weight): npers * 258 rounded up to 16 for the fp32 LDS-DMA GEMM, to 32 for
    the split GEMM (K % 32 == 0): 528 / 272 and 544 / 288."""
    m = 32 if precision == "fp32_split" else 16
    return (int(npers) * (NFEATS - 4) + m - 1) // m * m


def split_twin_layout(N, K):
    """Host: how the fp16-plane twin of an fp32 weight [N, K] is stored -- {"shape": (2, N, K), "plane_stride": N * K, "packed": fragment order or not}.
    Fragment order wherever the packed split GEMM covers the shape (N % 64 == 0 and K % 64 == 0), plain planes otherwise (the embed weight: K = 544 / 288)."""
    if K % 32:
        raise ValueError(f"split twin of a [{N}, {K}] weight: the split GEMM needs K % 32 == 0")
    return {"shape": (2, int(N), int(K)), "plane_stride": int(N) * int(K), "packed": N % 64 == 0 and K % 64 == 0}


def interclip_split_twins(cfg):
    """Host: name -> split_twin_layout of every weight twin InterCLIP(cfg, precision="fp32_split") builds in load_state_dict: the embed weight zero-padded to
    Kp, the four GEMM matrices of every motion and text layer (one storage order per layer: fragment order iff D % 64 == 0 and F % 64 == 0), and both output
    Linears."""
    D, F, L = int(cfg["LATENT_DIM"]), int(cfg["FF_SIZE"]), int(cfg["NUM_LAYERS"])
    out = {"motion_encoder.embed_motion.weight": split_twin_layout(D, embed_k_pad(_npers(cfg), "fp32_split"))}

    def stack(prefix, n, d):
        packed = d % 64 == 0 and F % 64 == 0
        for i in range(n):
            for k, (N, K) in (("self_attn.in_proj_weight", (3 * d, d)), ("self_attn.out_proj.weight", (d, d)), ("linear1.weight", (F, d)), ("linear2.weight", (d, F))):
                out[f"{prefix}layers.{i}.{k}"] = dict(split_twin_layout(N, K), packed=packed)
    stack("motion_encoder.transformer.", L, D)
    stack("textTransEncoder.", TEXT_LAYERS, TEXT_DIM)
    out["motion_encoder.out.weight"] = split_twin_layout(EMB_DIM, D)
    out["out.weight"] = split_twin_layout(EMB_DIM, TEXT_DIM)
    return out


def strip_model_prefix(state_dict):
    """The key renaming of build_models (utils.py:118-121): every key that contains "model" has "model." removed."""
    return {(k.replace("model.", "") if "model" in k else k): v for k, v in state_dict.items()}


def _enc_shapes(prefix, layers, D, F):
    s = {}
    for i in range(layers):
        q = f"{prefix}layers.{i}."
        s.update({q + "self_attn.in_proj_weight": (3 * D, D), q + "self_attn.in_proj_bias": (3 * D,), q + "self_attn.out_proj.weight": (D, D),
                  q + "self_attn.out_proj.bias": (D,), q + "linear1.weight": (F, D), q + "linear1.bias": (F,), q + "linear2.weight": (D, F),
                  q + "linear2.bias": (D,), q + "norm1.weight": (D,), q + "norm1.bias": (D,), q + "norm2.weight": (D,), q + "norm2.bias": (D,)})
    return s


def interclip_shapes(cfg, vocab=None, context=None):
    """name -> shape of InterCLIP(cfg).state_dict() without the pe buffer.  vocab / context None: any size (they belong to the CLIP checkpoint)."""
    D, F, L = int(cfg["LATENT_DIM"]), int(cfg["FF_SIZE"]), int(cfg["NUM_LAYERS"])
    npers = _npers(cfg)
    s = {"motion_encoder.query_token": (1, D), "motion_encoder.embed_motion.weight": (D, npers * int(cfg["INPUT_DIM"])),
         "motion_encoder.embed_motion.bias": (D,)}
    s.update(_enc_shapes("motion_encoder.transformer.", L, D, F))
    s.update({"motion_encoder.out_ln.weight": (D,), "motion_encoder.out_ln.bias": (D,), "motion_encoder.out.weight": (EMB_DIM, D),
              "motion_encoder.out.bias": (EMB_DIM,), "token_embedding.weight": (vocab, TEXT_DIM), "positional_embedding": (context, TEXT_DIM),
              "latent_scale": (1,)})
    s.update(_enc_shapes("textTransEncoder.", TEXT_LAYERS, TEXT_DIM, F))
    s.update({"text_ln.weight": (TEXT_DIM,), "text_ln.bias": (TEXT_DIM,), "out.weight": (EMB_DIM, TEXT_DIM), "out.bias": (EMB_DIM,)})
    return s


def _npers(cfg):
    mode = cfg["MODE"]
    if mode not in ("interaction", "individual"):
        raise ValueError(f"InterCLIP: MODE {mode!r} not recognized (interaction / individual)")
    return 2 if mode == "interaction" else 1


class InterCLIP:
    """InterCLIP(cfg) of src/evaluation/models.py for inference: ``encode_motion`` / ``encode_text`` fill ``batch["motion_emb"]`` /
    ``batch["text_emb"]``.  cfg: the keys of configs/eval.yaml (a mapping or a configs.CfgNode)."""

    def __init__(self, cfg, device="cuda", precision="fp32"):
        if precision not in PRECISIONS:
            raise ValueError(f"InterCLIP: precision {precision!r} not recognized ({' / '.join(PRECISIONS)})")
        self.cfg = cfg
        self.device = torch.device(device)
        self.precision = precision
        self.split = precision == "fp32_split"
        self.mode = cfg["MODE"]
        self.npers = _npers(cfg)
        if int(cfg["INPUT_DIM"]) != NFEATS - 4:
            raise ValueError(f"InterCLIP: INPUT_DIM must be {NFEATS - 4} (the {NFEATS} pose features of a person without the last 4), got {cfg['INPUT_DIM']}")
        if cfg["ACTIVATION"] != "gelu":
            raise ValueError(f"InterCLIP: ACTIVATION {cfg['ACTIVATION']!r} is not supported (gelu)")
        self.D, self.F, self.L, self.H = int(cfg["LATENT_DIM"]), int(cfg["FF_SIZE"]), int(cfg["NUM_LAYERS"]), int(cfg["NUM_HEADS"])
        self.K = self.npers * (NFEATS - 4)
        # the fp32 LDS-DMA GEMM path wants K % 16 == 0, the split GEMM K % 32 == 0: A and the weight are zero-padded alike
        self.k_pad = embed_k_pad(self.npers, precision)
        if self.split:
            if self.D % self.H or self.D // self.H not in (64, 128):
                raise ValueError(f"InterCLIP: precision 'fp32_split' needs a motion-encoder head size of 64 or 128 (the ragged split layer), got "
                                 f"LATENT_DIM / NUM_HEADS = {self.D} / {self.H} = head size {self.D / self.H:g}")
            if self.D % 32 or self.F % 32:
                raise ValueError(f"InterCLIP: precision 'fp32_split' needs LATENT_DIM and FF_SIZE to be multiples of 32, got {self.D} and {self.F}")
        self._w = None

    # ---- weights -------------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=True):
        """sd: the reference's names (InterCLIP.state_dict(); a checkpoint's "model." prefix is removed by strip_model_prefix).  The buffer
        motion_encoder.sequence_pos_encoder.pe is accepted and ignored (recomputed).  Every check runs on the host before anything is copied
        to the device."""
        want = interclip_shapes(self.cfg)
        unexpected = sorted(k for k in sd if k not in want and k != PE_KEY)
        missing = sorted(k for k in want if k not in sd)
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for InterCLIP:\n\tMissing key(s): %s\n\tUnexpected key(s): %s" % (missing[:8], unexpected[:8]))
        for k, shape in want.items():
            if k not in sd:
                continue
            got = tuple(sd[k].shape)
            if len(got) != len(shape) or any(w is not None and g != w for g, w in zip(got, shape)):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {got}, the shape in current model is "
                                   f"{tuple('*' if w is None else w for w in shape)}")
        if missing:
            raise RuntimeError("InterCLIP.load_state_dict(strict=False): the encoders cannot run without %s" % missing[:8])
        g = lambda k: torch.as_tensor(sd[k]).detach().to(device=self.device, dtype=torch.float32).contiguous()
        layers = lambda p, n: [{k.replace("self_attn.", ""): g(f"{p}layers.{i}.{k}") for k in _ENC_KEYS} for i in range(n)]
        w = {"query": g("motion_encoder.query_token"), "embed_b": g("motion_encoder.embed_motion.bias"),
             "m_layers": layers("motion_encoder.transformer.", self.L), "out_ln_w": g("motion_encoder.out_ln.weight"),
             "out_ln_b": g("motion_encoder.out_ln.bias"), "m_out_w": g("motion_encoder.out.weight"), "m_out_b": g("motion_encoder.out.bias"),
             "table": g("token_embedding.weight"), "pos": g("positional_embedding"), "scale": g("latent_scale"),
             "t_layers": layers("textTransEncoder.", TEXT_LAYERS), "text_ln_w": g("text_ln.weight"), "text_ln_b": g("text_ln.bias"),
             "t_out_w": g("out.weight"), "t_out_b": g("out.bias")}
        ew = torch.zeros(self.D, self.k_pad, device=self.device, dtype=torch.float32)
        ew[:, :self.K] = g("motion_encoder.embed_motion.weight")
        w["embed_w"] = ew
        w["pe"] = pe_table(self.D, max_len=2000).to(self.device).contiguous()          # MotionEncoder: PositionalEncoding(max_len=2000)
        if self.split:          # the fp16-plane twins, once: embed (plain planes: Kp % 64 != 0), the layers and both output Linears
            w["embed_s"] = ops.split_weight(ew, pack=False)[0]
            w["m_layers_s"] = [ops.encoder_layer_split_weights(lw) for lw in w["m_layers"]]
            w["t_layers_s"] = [ops.encoder_layer_split_weights(lw) for lw in w["t_layers"]]
            w["m_out_s"], w["m_out_packed"] = ops.split_weight(w["m_out_w"])
            w["t_out_s"], w["t_out_packed"] = ops.split_weight(w["t_out_w"])
        self._w = w
        return self

    def _weights(self):
        if self._w is None:
            raise RuntimeError("InterCLIP: no weights loaded (load_state_dict)")
        return self._w

    # ---- motion ------------------------------------------------------------------------------------------------------------------------
    def sequence_layout(self, T, motion_lens):
        """Host: the packed token sequences of a batch -- (seq_off, seq_len) int32 arrays, total rows, longest sequence."""
        lens = [int(v) for v in np.asarray(torch.as_tensor(motion_lens).cpu()).reshape(-1)]
        for i, n in enumerate(lens):
            if n < 1:
                raise ValueError(f"encode_motion: item {i} has motion_lens = {n}; every motion needs at least one frame")
        seq_len = np.array([1 + min(int(T), n) for n in lens], dtype=np.int32)
        seq_off = np.concatenate([[0], np.cumsum(seq_len)[:-1]]).astype(np.int32)
        return seq_off, seq_len, int(seq_len.sum()), int(seq_len.max())

    def _motion_args(self, batch, who, width):
        """The checked inputs of an encode_motion call: (motions fp32 on the device [B, T, width], the batch's sequence layout on the host)."""
        motions = torch.as_tensor(batch["motions"]).to(device=self.device, dtype=torch.float32)
        if motions.dim() != 3 or motions.shape[2] != width:
            raise ValueError(f"{who}: motions [B, T, {width}] expected, got {tuple(motions.shape)}")
        if motions.stride(2) != 1:
            motions = motions.contiguous()
        return motions, self.sequence_layout(motions.shape[1], batch["motion_lens"])

    def _encode_packed(self, a, seq_off, seq_len, total, longest):
        """From the embedding GEMM's A operand [total, k_pad] of packed token sequences to their embeddings [nseq, 512]."""
        w = self._weights()
        h = ops.linear(a, w["embed_w"], w["embed_b"])
        ops.motion_tokens_(h, w["query"], w["pe"], seq_off, seq_len, longest)
        ws = torch.empty(ops.load_library().mmdm_encoder_layer_workspace(1, total, self.D, self.F), device=self.device, dtype=torch.float32)
        for lw in w["m_layers"]:
            ops.encoder_layer_ragged_(h, lw, self.H, seq_off, seq_len, longest, activation="gelu", eps=1e-5, workspace=ws)
        tok = ops.gather_rows(h, seq_off)
        tok = ops.layernorm(tok, w["out_ln_w"], w["out_ln_b"], 1e-5)
        emb = ops.linear(tok, w["m_out_w"], w["m_out_b"])
        return ops.l2_normalize(emb, w["scale"])

    def _encode_packed_split(self, a, seq_off, seq_len, total, longest):
        """_encode_packed in the fp32_split mode: a = the A operand as fp16 planes [2, total, k_pad].  Row kernels: build 1 (what a precision-2 handle runs)."""
        w = self._weights()
        h = ops.linear_split(a, w["embed_s"], w["embed_b"])
        h, hs = ops.motion_tokens_split_(h, w["query"], w["pe"], seq_off, seq_len, longest, build=1)
        ws = torch.empty(ops.load_library().mmdm_encoder_layer_split_workspace(1, total, self.D, self.F), device=self.device, dtype=torch.float32)
        for i, lw in enumerate(w["m_layers_s"]):
            ops.encoder_layer_ragged_split_(h, hs, lw, self.H, seq_off, seq_len, longest, eps=1e-5, last=i + 1 == self.L, workspace=ws)
        tok = ops.gather_rows(h, seq_off)
        _, toks = ops.layernorm_split(tok, w["out_ln_w"], w["out_ln_b"], 1e-5, build=1)
        emb = ops.linear_split(toks, w["m_out_s"], w["m_out_b"], packed=w["m_out_packed"])
        return ops.l2_normalize(emb, w["scale"], build=1)

    def encode_motion(self, batch):
        """batch["motions"] [B, T, npers * 262], batch["motion_lens"] [B] -> batch["motion_emb"] [B, 512] (models.py:144-154, 50-80)."""
        self._weights()
        motions, (off_h, len_h, total, longest) = self._motion_args(batch, "encode_motion", self.npers * NFEATS)
        if len(off_h) != motions.shape[0]:
            raise ValueError(f"encode_motion: {motions.shape[0]} motions but {len(off_h)} lengths")
        seq_off = torch.from_numpy(off_h).to(self.device)
        seq_len = torch.from_numpy(len_h).to(self.device)
        if self.split:
            a = ops.motion_pack_split(motions, seq_off, seq_len, longest, total, npers=self.npers, k_pad=self.k_pad, build=1)
            batch["motion_emb"] = self._encode_packed_split(a, seq_off, seq_len, total, longest)
            return batch
        a = ops.motion_pack(motions, seq_off, seq_len, longest, total, npers=self.npers, k_pad=self.k_pad)
        batch["motion_emb"] = self._encode_packed(a, seq_off, seq_len, total, longest)
        return batch

    def encode_motion_individual(self, batch):
        """MODE: individual only.  batch["motions"] [B, T, 524] (both persons of an interaction), batch["motion_lens"] [B] -> batch["motion_emb"] [2B, 512] in
        the order p1 of item 0, p2 of item 0, p1 of item 1, ... -- what EvaluatorModelWrapperIndividual (src/evaluation/utils.py:284-315) hands its encoder:
        every person centred on its own with smpl_to_ih(center_motion(ih_to_smpl(.))) over the WHOLE buffer handed in (the floor is the minimum over all T
        frames, padding included: ops.center_motion), interleaved at batch level, lengths repeated.  Centring and packing are one pass (ops.center_pack); the
        padded [2B, T, 262] tensor is never formed.  The cross product of the facing runs along the last dimension for every B (the reference's
        torch.cross without dim goes wrong at a per-call batch of exactly 3: not reproduced)."""
        if self.mode != "individual":
            raise ValueError(f"encode_motion_individual: the model's MODE is {self.mode!r}; the per-person encoding needs MODE 'individual'")
        self._weights()
        motions, (off_h, len_h, _, longest) = self._motion_args(batch, "encode_motion_individual", 2 * NFEATS)
        if len(off_h) != motions.shape[0]:
            raise ValueError(f"encode_motion_individual: {motions.shape[0]} motions but {len(off_h)} lengths")
        len_h = np.repeat(len_h, 2)
        off_h = np.concatenate([[0], np.cumsum(len_h)[:-1]]).astype(np.int32)
        total = int(len_h.sum())
        seq_off = torch.from_numpy(off_h).to(self.device)
        seq_len = torch.from_numpy(len_h).to(self.device)
        if self.split:
            a = ops.center_pack_split(motions, seq_off, seq_len, longest, total, k_pad=self.k_pad)
            batch["motion_emb"] = self._encode_packed_split(a, seq_off, seq_len, total, longest)
            return batch
        a = ops.center_pack(motions, seq_off, seq_len, longest, total, k_pad=self.k_pad)
        batch["motion_emb"] = self._encode_packed(a, seq_off, seq_len, total, longest)
        return batch

    # ---- text --------------------------------------------------------------------------------------------------------------------------
    def encode_text(self, batch):
        """batch["tokens_text"] (token ids [B, L]) or batch["text"] (prompts; needs the ``clip`` package) -> batch["text_emb"] [B, 512]
        (models.py:156-180).  No mask, as in the reference."""
        w = self._weights()
        tokens = torch.as_tensor(batch["tokens_text"]) if "tokens_text" in batch else tokenize(list(batch["text"]))
        tok = tokens.to(device=self.device, dtype=torch.int32).contiguous()
        x = ops.token_embed(w["table"], tok, w["pos"], build=1 if self.split else 0)
        if self.split:          # the uniform split layer; 768 / 8 = 96-wide heads: its fp32 attention.  The planes of the embedded tokens are layer 0's operand.
            xs = ops.split_f32(x)
            ws = torch.empty(ops.load_library().mmdm_encoder_layer_split_workspace(x.shape[0], x.shape[1], TEXT_DIM, self.F), device=self.device, dtype=torch.float32)
            for i, lw in enumerate(w["t_layers_s"]):
                ops.encoder_layer_split_(x, xs, lw, TEXT_HEADS, eps=1e-5, last=i + 1 == TEXT_LAYERS, workspace=ws)
            _, eots = ops.layernorm_split(_eot_rows(tokens, x), w["text_ln_w"], w["text_ln_b"], 1e-5, build=1)      # LayerNorm is per row: the EOT rows only
            out = ops.linear_split(eots, w["t_out_s"], w["t_out_b"], packed=w["t_out_packed"])
            batch["text_emb"] = ops.l2_normalize(out, w["scale"], build=1)
            return batch
        ws = None
        for lw in w["t_layers"]:
            ops.encoder_layer_(x, lw, TEXT_HEADS, norm_first=False, activation="gelu", causal=False, eps=1e-5, workspace=ws)
        x = ops.layernorm(x, w["text_ln_w"], w["text_ln_b"], 1e-5)
        out = ops.linear(_eot_rows(tokens, x), w["t_out_w"], w["t_out_b"])
        batch["text_emb"] = ops.l2_normalize(out, w["scale"])
        return batch


class EvaluatorModelWrapper:
    """EvaluatorModelWrapper of src/evaluation/utils.py:126-235.  cfg_or_model: an InterCLIP with its weights loaded, or a cfg whose CHECKPOINT
    names a checkpoint file (loaded as build_models does; ``precision`` is InterCLIP's and applies to that case only: a model handed in keeps its own)."""

    def __init__(self, cfg_or_model, device="cuda", precision="fp32"):
        if isinstance(cfg_or_model, InterCLIP):
            self.model = cfg_or_model
        else:
            cfg = cfg_or_model
            ckpt = torch.load(cfg["CHECKPOINT"], map_location="cpu")
            self.model = InterCLIP(cfg, device=device, precision=precision).load_state_dict(strip_model_prefix(ckpt["state_dict"]), strict=True)
        self.cfg = self.model.cfg
        self.device = self.model.device
        self.extended = bool(self.cfg.get("EXTENDED", False))

    def _batch(self, batch_data):
        text, motion1, motion2, motion_lens = batch_data[1], batch_data[2], batch_data[3], batch_data[4]
        f = lambda m: torch.as_tensor(np.asarray(m) if not torch.is_tensor(m) else m).detach().float()
        motions = torch.cat([f(motion1), f(motion2)], dim=-1)
        motion_lens = torch.as_tensor(np.asarray(motion_lens) if not torch.is_tensor(motion_lens) else motion_lens).reshape(-1).cpu()
        align_idx = np.argsort(motion_lens.tolist())[::-1].copy()          # utils.py:164 -- numpy on the host, exactly so
        motions = motions[torch.from_numpy(align_idx)]
        motion_lens = motion_lens[torch.from_numpy(align_idx)]
        B, T = motions.shape[:2]
        padded_len = max(min(T, int(n)) for n in motion_lens)
        batch = {"motions": motions.reshape(B, T, -1)[:, :padded_len], "motion_lens": motion_lens}
        if torch.is_tensor(text) or isinstance(text, np.ndarray):
            batch["tokens_text"] = torch.as_tensor(text)
        elif text is not None:
            batch["text"] = list(text)
        return batch, align_idx

    def get_co_embeddings(self, batch_data):
        """(name, text, motion1, motion2, motion_lens[, text_individual1, text_individual2]) -> (text_embedding, motion_embedding), both in the
        order np.argsort(motion_lens)[::-1].  `text` may be a tensor of token ids [B, L] in place of the prompts."""
        with torch.no_grad():
            batch, align_idx = self._batch(batch_data)
            motion_embedding = self.model.encode_motion(batch)["motion_emb"]
            text_embedding = self.model.encode_text(batch)["text_emb"][torch.from_numpy(align_idx).to(self.device)]
        return text_embedding, motion_embedding

    def get_motion_embeddings(self, batch_data):
        with torch.no_grad():
            batch, _ = self._batch(batch_data)
            return self.model.encode_motion(batch)["motion_emb"]


class EvaluatorModelWrapperIndividual:
    """EvaluatorModelWrapperIndividual of src/evaluation/utils.py:237-383: every person of an interaction is scored as a motion of its own against its own
    prompt by an InterCLIP in MODE: individual.  cfg_or_model as in EvaluatorModelWrapper.  No length sort: embeddings come in the order p1 of item 0,
    p2 of item 0, p1 of item 1, ...; the centring is InterCLIP.encode_motion_individual's (over the whole buffer handed in)."""
    individual = True

    def __init__(self, cfg_or_model, device="cuda", precision="fp32"):
        if isinstance(cfg_or_model, InterCLIP):
            self.model = cfg_or_model
        else:
            cfg = cfg_or_model
            ckpt = torch.load(cfg["CHECKPOINT"], map_location="cpu")
            self.model = InterCLIP(cfg, device=device, precision=precision).load_state_dict(strip_model_prefix(ckpt["state_dict"]), strict=True)
        if self.model.mode != "individual":
            raise ValueError(f"EvaluatorModelWrapperIndividual: the model's MODE is {self.model.mode!r}; it needs MODE 'individual'")
        self.cfg = self.model.cfg
        self.device = self.model.device
        self.extended = bool(self.cfg.get("EXTENDED", False))

    @staticmethod
    def _motion_batch(batch_data):
        motion1, motion2, motion_lens = batch_data[2], batch_data[3], batch_data[4]
        f = lambda m: torch.as_tensor(np.asarray(m) if not torch.is_tensor(m) else m).detach().float()
        motion_lens = torch.as_tensor(np.asarray(motion_lens) if not torch.is_tensor(motion_lens) else motion_lens).reshape(-1).cpu()
        return {"motions": torch.cat([f(motion1), f(motion2)], dim=-1), "motion_lens": motion_lens}

    @staticmethod
    def _text_batch(batch_data):
        if len(batch_data) < 7 or batch_data[5] is None or batch_data[6] is None:
            raise ValueError("EvaluatorModelWrapperIndividual.get_co_embeddings: the batch carries no text_individual1 / text_individual2 "
                             "(name, text, motion1, motion2, motion_lens, text_individual1, text_individual2): the dataset must be built with EXTENDED: True")
        t1, t2 = batch_data[5], batch_data[6]
        if torch.is_tensor(t1) or isinstance(t1, np.ndarray):
            t1, t2 = torch.as_tensor(t1), torch.as_tensor(t2)
            return {"tokens_text": torch.stack([t1, t2], dim=1).reshape(2 * t1.shape[0], -1)}
        t1, t2 = list(t1), list(t2)
        return {"text": [t1[i // 2] if i % 2 == 0 else t2[i // 2] for i in range(2 * len(t1))]}          # utils.py:282

    def get_co_embeddings(self, batch_data):
        """(name, text, motion1, motion2, motion_lens, text_individual1, text_individual2) -> (text_embedding, motion_embedding), both [2B, 512] in the
        interleaved order.  text_individual1 / 2 may be tensors of token ids [B, L] in place of the prompts."""
        with torch.no_grad():
            text = self._text_batch(batch_data)
            motion_embedding = self.model.encode_motion_individual(self._motion_batch(batch_data))["motion_emb"]
            text_embedding = self.model.encode_text(text)["text_emb"]
        return text_embedding, motion_embedding

    def get_motion_embeddings(self, batch_data):
        with torch.no_grad():
            return self.model.encode_motion_individual(self._motion_batch(batch_data))["motion_emb"]


# ---- metrics (float64 numpy / scipy on the host) ---------------------------------------------------------------------------------------
def euclidean_distance_matrix(matrix1, matrix2):
    """dist[i, j] = ||matrix1[i] - matrix2[j]||_2 through the expansion -2 a.b + |a|^2 + |b|^2, summed in that order."""
    assert matrix1.shape[1] == matrix2.shape[1]
    cross = -2 * np.dot(matrix1, matrix2.T)
    sq1 = np.sum(np.square(matrix1), axis=1, keepdims=True)
    sq2 = np.sum(np.square(matrix2), axis=1)
    return np.sqrt(cross + sq1 + sq2)


def calculate_top_k(mat, top_k):
    """mat [N, N]: row i lists candidate indices by rank; out[i, k] = (i is among the first k + 1 of row i)."""
    n = mat.shape[0]
    hit = mat[:, :top_k] == np.arange(n)[:, None]
    return np.cumsum(hit, axis=1) > 0


def calculate_R_precision(embedding1, embedding2, top_k, sum_all=False):
    ranks = np.argsort(euclidean_distance_matrix(embedding1, embedding2), axis=1)
    top = calculate_top_k(ranks, top_k)
    return top.sum(axis=0) if sum_all else top


def calculate_matching_score(embedding1, embedding2, sum_all=False):
    assert embedding1.ndim == 2 and embedding1.shape == embedding2.shape
    from scipy import linalg
    dist = linalg.norm(embedding1 - embedding2, axis=1)
    return dist.sum(axis=0) if sum_all else dist


def calculate_activation_statistics(activations):
    """(mean [D], covariance [D, D]) of emb_scale * activations [N, D]."""
    a = activations * emb_scale
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def calculate_diversity(activation, diversity_times):
    """Mean half-distance between two random draws (np.random, without replacement each) of `diversity_times` scaled activations."""
    assert activation.ndim == 2 and activation.shape[0] > diversity_times
    from scipy import linalg
    n = activation.shape[0]
    a = activation * emb_scale
    first = np.random.choice(n, diversity_times, replace=False)
    second = np.random.choice(n, diversity_times, replace=False)
    return linalg.norm((a[first] - a[second]) / 2, axis=1).mean()


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Frechet distance of two Gaussians: |mu1 - mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)); a singular product gets eps on both diagonals."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def calculate_multimodality(activation, multimodality_times):
    """activation [N, R, D]: mean distance between two random draws (np.random) of `multimodality_times` of every prompt's R repeats."""
    assert activation.ndim == 3 and activation.shape[1] > multimodality_times
    from scipy import linalg
    r = activation.shape[1]
    first = np.random.choice(r, multimodality_times, replace=False)
    second = np.random.choice(r, multimodality_times, replace=False)
    return linalg.norm(activation[:, first] - activation[:, second], axis=2).mean()


# ---- the evaluation pass ---------------------------------------------------------------------------------------------------------------
def _text_of(items):
    if all("tokens_text" in d for d in items):
        return torch.stack([torch.as_tensor(d["tokens_text"]).reshape(-1) for d in items])
    return [d["text"] for d in items]


def _batches(items, batch_size):
    items = list(items)
    for i in range(0, len(items), batch_size):
        chunk = items[i:i + batch_size]
        yield ("generated", _text_of(chunk), np.stack([np.asarray(d["motion1"]) for d in chunk]), np.stack([np.asarray(d["motion2"]) for d in chunk]),
               torch.as_tensor([int(d["motion_lens"]) for d in chunk]))


def _individual_text_of(items, k):
    if all(f"tokens_individual{k}" in d for d in items):
        return torch.stack([torch.as_tensor(d[f"tokens_individual{k}"]).reshape(-1) for d in items])
    if all(f"text_individual{k}" in d for d in items):
        return [d[f"text_individual{k}"] for d in items]
    return None


def _batches_individual(items, batch_size):
    """The 7-tuples of the individual wrapper; the two individual texts are None where the items carry none (the wrapper refuses them by name)."""
    items = list(items)
    for i in range(0, len(items), batch_size):
        chunk = items[i:i + batch_size]
        yield ("generated", None, np.stack([np.asarray(d["motion1"]) for d in chunk]), np.stack([np.asarray(d["motion2"]) for d in chunk]),
               torch.as_tensor([int(d["motion_lens"]) for d in chunk]), _individual_text_of(chunk, 1), _individual_text_of(chunk, 2))


def evaluate_generated(wrapper, generated, mm_generated=(), groundtruth=None, batch_size=32, diversity_times=125, mm_num_times=5):
    """Scores the lists generate_for_evaluation returns, the way evaluate_matching_score / evaluate_fid / evaluate_diversity /
    evaluate_multimodality do (scripts/eval/mixermdm.py:17-114; the defaults are that script's constants).  generated / groundtruth: lists of
    {"motion1", "motion2" [T, 262], "motion_lens", "text" or "tokens_text"}; mm_generated: lists of {"mm_motions" [R, T, 2, 262], "motion_lens",
    ...}.  Batches of `batch_size` in list order; a last partial batch is scored too (the reference's DataLoader drops it).
    Returns {"mm_dist", "r_precision" [top 1..3], "diversity", "multimodality", and "fid" when groundtruth is given}; "diversity" is None when
    there are not more than `diversity_times` motions.  The two sampled metrics draw from np.random.  The fp32 embeddings are widened to float64
    before any metric is formed (the reference hands its functions the fp32 arrays).
    An EvaluatorModelWrapperIndividual (``wrapper.individual``) scores every person on its own: the items carry "text_individual1" / "text_individual2" (or
    "tokens_individual1" / "tokens_individual2"), and every metric is formed over the 2B embeddings of a batch, as the reference's evaluation() does with
    that wrapper."""
    if getattr(wrapper, "individual", False):
        return _evaluate_generated_individual(wrapper, generated, mm_generated, groundtruth, batch_size, diversity_times, mm_num_times)
    mm_sum, top_k, n, acts = 0.0, np.zeros(3), 0, []
    for batch in _batches(generated, batch_size):
        text_emb, motion_emb = wrapper.get_co_embeddings(batch)
        t, m = text_emb.double().cpu().numpy(), motion_emb.double().cpu().numpy()
        dist = euclidean_distance_matrix(t, m)
        mm_sum += dist.trace()
        top_k = top_k + calculate_top_k(np.argsort(dist, axis=1), top_k=3).sum(axis=0)
        n += t.shape[0]
        acts.append(m)
    if not n:
        raise ValueError("evaluate_generated: no generated motions")
    acts = np.concatenate(acts, axis=0)
    out = {"mm_dist": float(mm_sum / n), "r_precision": top_k / n}
    if groundtruth is not None:
        gt = np.concatenate([wrapper.get_motion_embeddings(b).double().cpu().numpy() for b in _batches(groundtruth, batch_size)], axis=0)
        gt_mu, gt_cov = calculate_activation_statistics(gt)
        mu, cov = calculate_activation_statistics(acts)
        out["fid"] = calculate_frechet_distance(gt_mu, gt_cov, mu, cov)
    out["diversity"] = calculate_diversity(acts, diversity_times) if acts.shape[0] > diversity_times else None
    mm = []
    for d in mm_generated:
        mo = np.asarray(d["mm_motions"])
        lens = torch.as_tensor([int(d["motion_lens"])] * mo.shape[0])
        mm.append(wrapper.get_motion_embeddings(("mm_generated", None, mo[:, :, 0], mo[:, :, 1], lens)).unsqueeze(0))
    out["multimodality"] = calculate_multimodality(torch.cat(mm, dim=0).double().cpu().numpy(), mm_num_times) if mm else 0
    return out


def _evaluate_generated_individual(wrapper, generated, mm_generated, groundtruth, batch_size, diversity_times, mm_num_times):
    """evaluate_generated with the individual wrapper: the same metrics over the 2B per-person embeddings of every batch."""
    mm_sum, top_k, n, acts = 0.0, np.zeros(3), 0, []
    for batch in _batches_individual(generated, batch_size):
        text_emb, motion_emb = wrapper.get_co_embeddings(batch)
        t, m = text_emb.double().cpu().numpy(), motion_emb.double().cpu().numpy()
        dist = euclidean_distance_matrix(t, m)
        mm_sum += dist.trace()
        top_k = top_k + calculate_top_k(np.argsort(dist, axis=1), top_k=3).sum(axis=0)
        n += t.shape[0]
        acts.append(m)
    if not n:
        raise ValueError("evaluate_generated: no generated motions")
    acts = np.concatenate(acts, axis=0)
    out = {"mm_dist": float(mm_sum / n), "r_precision": top_k / n}
    if groundtruth is not None:
        gt = np.concatenate([wrapper.get_motion_embeddings(b).double().cpu().numpy() for b in _batches_individual(groundtruth, batch_size)], axis=0)
        gt_mu, gt_cov = calculate_activation_statistics(gt)
        mu, cov = calculate_activation_statistics(acts)
        out["fid"] = calculate_frechet_distance(gt_mu, gt_cov, mu, cov)
    out["diversity"] = calculate_diversity(acts, diversity_times) if acts.shape[0] > diversity_times else None
    mm = []
    for d in mm_generated:
        mo = np.asarray(d["mm_motions"])
        lens = torch.as_tensor([int(d["motion_lens"])] * mo.shape[0])
        mm.append(wrapper.get_motion_embeddings(("mm_generated", None, mo[:, :, 0], mo[:, :, 1], lens)).unsqueeze(0))
    out["multimodality"] = calculate_multimodality(torch.cat(mm, dim=0).double().cpu().numpy(), mm_num_times) if mm else 0
    return out


# ---- replications and the F-score (scripts/eval/mixermdm.py:117-121, 216-241) ------------------------------------------------------------------
def summarize_replications(metric_dicts):
    """[{metric: value}, ...] of several replications -> {metric: {"mean", "conf_interval"}} with conf_interval = 1.96 * std / sqrt(n) (get_metric_statistics:
    np.mean / np.std over the replications, element-wise for the R-precision array).  A metric that is None in any replication is left out."""
    metric_dicts = list(metric_dicts)
    if not metric_dicts:
        raise ValueError("summarize_replications: no replications")
    out = {}
    for k in metric_dicts[0]:
        vals = [d[k] for d in metric_dicts]
        if any(v is None for v in vals):
            continue
        v = np.asarray(vals, dtype=np.float64)
        out[k] = {"mean": np.mean(v, axis=0), "conf_interval": 1.96 * np.std(v, axis=0) / np.sqrt(v.shape[0])}
    return out


def f_score_summary(summary_interaction, summary_individual):
    """The harmonic mean of interaction and individual quality (calculate_f_score): per metric of both summaries (summarize_replications' layout),
    {"f_score": 2 a b / (a + b), "conf_interval": (ci_a + ci_b) / 2} of the means a, b and the intervals, element-wise for R-precision; where both means
    are 0 the F-score is 0.  Metrics that only one summary holds are left out.  Returns a dictionary; writes no log file."""
    out = {}
    for k, si in summary_interaction.items():
        if k not in summary_individual:
            continue
        a, b = np.asarray(si["mean"], dtype=np.float64), np.asarray(summary_individual[k]["mean"], dtype=np.float64)
        ca, cb = np.asarray(si["conf_interval"], dtype=np.float64), np.asarray(summary_individual[k]["conf_interval"], dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(a + b == 0, 0.0, 2 * a * b / (a + b))          # two zero means (an R-precision of 0 on both sides): 0, where the reference prints nan
        out[k] = {"f_score": f if f.ndim else np.float64(f), "conf_interval": (cb + ca) / 2}
    return out
