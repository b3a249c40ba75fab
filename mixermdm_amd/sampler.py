"""Python owner of an mmdm_handle (include/mmdm.h section 2): weights, schedule, the DDIM host loop.

The loop itself is one C call per chunk of steps (``mmdm_run``), optionally replaying a captured hipGraph; Python only
decides how many steps to run and where the history buffers live.
"""
import ctypes as C
import numpy as np
import torch

from ._lib import Config, BeginOptions, BeginRaggedOptions, MMDMError, load_library, check
from .schedule import make_schedule

STATS_ORDER = ("mean_hml", "std_hml", "mean_ih", "std_ih")


def pe_table(d_model, max_len=5000):
    """PositionalEncoding buffer, generated exactly like the reference (src/models/utils/utils.py:24-35) with torch on the
    host, then handed to the library as the ``sequence_pos_encoder.pe`` entry of the state dict."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-np.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def pack_ragged_options(lens, *, noise=None, seeds=None, noise_rows=None, x_start=None, init_image=None, skip_timesteps=0):
    """The options of a ragged call (Sampler.begin_ragged) as mmdm_begin_ragged_opts takes them -- buffers PACKED like x_T, the items' frames back
    to back -- from packed tensors or per-item lists; needs no device (tensors stay where they are).  -> dict(noise [n, sum(lens), 524] | None,
    seeds [B ints] | None, noise_rows [B ints] | None, x_start [sum(lens), 524] | None, init_image [sum(lens), 524] | None, skip_timesteps).
      noise       [n, sum(lens), 524], or B tensors [n, T_i, 524] (one n)
      seeds       B ints: every item its own call (noise_rows default to zeros); ONE int: the batch is one call (noise_rows default to range(B))
      noise_rows  B ints >= 0: the `b` of every item in the generator's counter; overrides the defaults; needs seeds
      x_start     [sum(lens), 524], or B tensors [T_i' >= T_i, 524], cut to T_i
      init_image  [sum(lens), 524], or B tensors [T_i, 524]
    Anything else is a ValueError."""
    lens = [int(v) for v in lens]
    B, total = len(lens), sum(lens)
    if B == 0 or min(lens) <= 0:
        raise ValueError(f"ragged options: lens {lens} (B >= 1 items of >= 1 frames)")
    f32 = lambda t: torch.as_tensor(t).to(torch.float32)

    def per_item(name, v):
        if len(v) != B:
            raise ValueError(f"ragged options: {name} lists {len(v)} items, the batch has {B}")
        return [f32(t) for t in v]

    if noise is not None and seeds is not None:
        raise ValueError("ragged options: give the step noise as a buffer (noise=) or as seeds (seeds=), not both")
    if noise_rows is not None and seeds is None:
        raise ValueError("ragged options: noise_rows count the generator's batch rows and need seeds=")
    if noise is not None:
        if isinstance(noise, (list, tuple)):
            parts = per_item("noise", noise)
            for b, t in enumerate(parts):
                if t.dim() != 3 or t.shape[0] != parts[0].shape[0] or tuple(t.shape[1:]) != (lens[b], 524):
                    raise ValueError(f"ragged options: noise of item {b}: [n, {lens[b]}, 524] with one n for all items expected, got {tuple(t.shape)}")
            noise = torch.cat(parts, 1)
        else:
            noise = f32(noise)
        if noise.dim() != 3 or tuple(noise.shape[1:]) != (total, 524):
            raise ValueError(f"ragged options: noise [steps, {total}, 524] expected, got {tuple(noise.shape)}")
        noise = noise.contiguous()
    if seeds is not None:
        if isinstance(seeds, (int, np.integer)):
            seeds, default_rows = [int(seeds)] * B, list(range(B))
        else:
            seeds, default_rows = [int(v) for v in seeds], [0] * B
            if len(seeds) != B:
                raise ValueError(f"ragged options: {len(seeds)} seeds for {B} items")
        seeds = [v & 0xFFFFFFFFFFFFFFFF for v in seeds]
        noise_rows = default_rows if noise_rows is None else [int(v) for v in noise_rows]
        if len(noise_rows) != B or min(noise_rows) < 0:
            raise ValueError(f"ragged options: noise_rows {noise_rows}: {B} ints >= 0 expected")
    if x_start is not None:
        if isinstance(x_start, (list, tuple)):
            parts = per_item("x_start", x_start)
            for b, t in enumerate(parts):
                if t.dim() != 2 or t.shape[0] < lens[b] or t.shape[1] != 524:
                    raise ValueError(f"ragged options: x_start of item {b}: [T' >= {lens[b]}, 524] expected, got {tuple(t.shape)}")
            x_start = torch.cat([t[:n] for t, n in zip(parts, lens)], 0)
        else:
            x_start = f32(x_start)
        if tuple(x_start.shape) != (total, 524):
            raise ValueError(f"ragged options: x_start [{total}, 524] expected, got {tuple(x_start.shape)}")
        x_start = x_start.contiguous()
    if init_image is not None:
        if isinstance(init_image, (list, tuple)):
            parts = per_item("init_image", init_image)
            for b, t in enumerate(parts):
                if tuple(t.shape) != (lens[b], 524):
                    raise ValueError(f"ragged options: init_image of item {b}: [{lens[b]}, 524] expected, got {tuple(t.shape)}")
            init_image = torch.cat(parts, 0)
        else:
            init_image = f32(init_image)
        if tuple(init_image.shape) != (total, 524):
            raise ValueError(f"ragged options: init_image [{total}, 524] expected, got {tuple(init_image.shape)}")
        init_image = init_image.contiguous()
    return dict(noise=noise, seeds=seeds, noise_rows=noise_rows, x_start=x_start, init_image=init_image, skip_timesteps=int(skip_timesteps))


def invert_steps(steps, S):
    """The number of reverse steps an inversion runs: None = all S; otherwise an int in [1, S] (ValueError)."""
    if steps is None:
        return int(S)
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= int(steps) <= S:
        raise ValueError(f"invert: steps={steps!r} outside [1, {S}] (None = all {S} steps of the schedule)")
    return int(steps)


def check_start_step(start_step, S, *, init_image=None, skip_timesteps=0):
    """start_step of sample_from / sample_ragged_from: the respaced step index in [0, S) whose level x_T is taken at -- the loop then runs start_step + 1
    steps (a partial inversion of k < S steps continues with start_step = k).  It is exclusive with init_image / skip_timesteps, which name the loop's first
    step themselves (ValueError)."""
    if isinstance(start_step, bool) or not isinstance(start_step, (int, np.integer)) or not 0 <= int(start_step) < S:
        raise ValueError(f"start_step={start_step!r} outside [0, {S})")
    if init_image is not None or skip_timesteps:
        raise ValueError("start_step is exclusive with init_image / skip_timesteps: both name the first step of the loop")
    return int(start_step)


class Sampler:
    """One handle = one device, one (max_batch, max_frames) workspace."""

    def __init__(self, *, d_latent, d_ff, d_layers, d_heads, m_latent=0, m_ff=0, m_layers=0, m_heads=1, mixing_mode=4, align=True,
                 xstart_align=True, model2_kind=0, force_influence_val=None, cfg_scale=3.5, max_batch=1, max_frames=300,
                 single_only=False, text_dim=768, device=None, cfg_scale_interaction=0.0, cfg_scale_individual=0.0, precision="fp32",
                 model1_kind=0, d1_latent=0, d1_ff=0, d1_layers=0, d1_heads=0, cfg_form=0):
        """single_only: False/0 = two-chain MixerMDM; True/1 = individual denoiser alone (2-way CFG);
        2 = interaction denoiser alone with the 4-way CFG of ClassifierFreeSampleModelMultiple;
        3 = in2IN "dual": both denoisers composed by ClassifierFreeSampleDualMDM (call set_dual_weights after set_schedule);
        4 = the InterGen denoiser alone under the 2-way CFG (needs model2_kind=1; cond [B, text_dim], x [B, T, 524]) -- the one single-chain mode whose
        begin / sample / begin_ragged / sample_ragged(_async) and set_eta take the loop's other arguments (eta, noise | seed(s), noise_rows, x_start,
        init_image, skip_timesteps) with the two-chain sampler's rules.
        cfg_form (single_only=4 only): the guidance wrapper of that one-chain sampler.  0 = the 2-way CFG above; 1 = the 4-way CFG of single_only=2
        (denoiser 2 alone, in2IN or InterGen by model2_kind; cond [B, 3*text_dim]); 2 = DualMDM as single_only=3 (cond [B, 5*text_dim]; set_dual_weights
        after set_schedule).  Forms 1 / 2 sample what single_only 2 / 3 sample, bit for bit, and take the loop's arguments and ragged batches as well.
        model1_kind: 0 = in2IN individual, 1 = MDMDenoiser (precision "fp32" or "fp32_split", the latter at head sizes 64 / 128; "bf16" /
        "bf16_fp8" are refused for it); d1_*: denoiser1's own sizes (0 = same as d_*).
        precision: "fp32" (native fp32 MFMA), "fp32_split" (fp32 results from six bf16 MFMAs per product on exactly split operands:
        same accuracy, the bf16 matrix rate), "bf16" (bf16 GEMM operands), "bf16_fp8" (BASELINE configs[4]: as "bf16" with the QKV /
        cross-attention input projections and both FFN GEMMs on fp8 e4m3 operands)."""
        if not torch.cuda.is_available():
            raise RuntimeError("mixermdm_amd.Sampler needs an MI355X (HIP device); there is no CPU path")
        self.lib = load_library()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.cfg = Config(d_latent, d_ff, d_layers, d_heads, m_latent, m_ff, m_layers, m_heads, 262, text_dim, mixing_mode, int(align),
                          int(xstart_align), model2_kind, int(force_influence_val is not None), float(force_influence_val or 0.0),
                          float(cfg_scale), max_batch, max_frames, int(single_only), float(cfg_scale_interaction), float(cfg_scale_individual),
                          {"fp32": 0, "bf16": 1, "fp32_split": 2, "bf16_fp8": 3}[precision], int(model1_kind), d1_latent, d1_ff, d1_layers, d1_heads,
                          int(cfg_form))
        self.single_only = int(single_only)
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_create(C.byref(self.cfg), C.byref(self.h)))
            # graph capture is not allowed on the legacy default stream: the handle works on its own stream
            self.stream = torch.cuda.Stream(device=self.device)
        self.schedule = None
        self._strategy = None
        self._hist = None
        self._parent = None
        self.lens, self.rows = None, 0

    def share(self, max_batch=None, max_frames=None):
        """A second Sampler over THIS sampler's weights (mmdm_create_shared): own workspace, stream, schedule tables and graph cache, one
        copy of the parameters.  K shared samplers keep K sampling calls in flight on K streams -- the reference's callers sample one
        item at a time (src/scripts/infer/mixermdm.py:184-188, src/evaluation/datasets.py:100-116), which leaves the GPU 40 % empty at B = 1.
        The weights must be loaded and prepared on `self`; load_state_dict / set_norm_stats / prepare are the parent's."""
        s = object.__new__(Sampler)
        s.lib, s.device, s.single_only = self.lib, self.device, self.single_only
        cfg = Config.from_buffer_copy(self.cfg)
        cfg.max_batch = int(max_batch or self.cfg.max_batch)
        cfg.max_frames = int(max_frames or self.cfg.max_frames)
        s.cfg = cfg
        s.h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_create_shared(self.h, cfg.max_batch, cfg.max_frames, C.byref(s.h)), self.h)
            s.stream = torch.cuda.Stream(device=self.device)
        s.schedule, s._strategy, s._hist, s._parent = None, None, None, self
        s.lens, s.rows = None, 0
        return s

    def close(self):
        """Frees the handle (mmdm_destroy selects the handle's own device before synchronising and freeing).  Tensors returned by
        state() are views of handle memory and are invalid afterwards."""
        if getattr(self, "h", None) and self.h.value:
            self.lib.mmdm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    # ---- weights ----------------------------------------------------------------------------------
    def load_state_dict(self, sd):
        """sd: Mixer state_dict (reference key names; src/models/mixermdm.py:134-148); strict: unknown keys raise here, missing
        keys raise in prepare().  pe buffers are regenerated if absent."""
        sd = dict(sd)
        D, Dm = self.cfg.d_latent, self.cfg.m_latent
        pes = []
        if self.single_only not in (2, 4) or self.cfg.cfg_form == 2:
            pes.append(("denoiser1.sequence_pos_encoder.pe", self.cfg.d1_latent or D))
        if self.single_only != 1:
            pes.append(("denoiser2.sequence_pos_encoder.pe", D))
        if self.single_only == 0:
            pes.append(("sequence_pos_encoder.pe", Dm))
        for k, d in pes:
            if k not in sd:
                sd[k] = pe_table(d)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        keep = []
        with torch.cuda.device(self.device):
            for k, v in sd.items():
                t = v.detach().to(device=self.device, dtype=torch.float32).contiguous()
                keep.append(t)
                rows, cols = (t.shape[0], 1) if t.dim() == 1 else (t.shape[0], t.shape[1])
                check(self.lib.mmdm_set_weight(self.h, k.encode(), C.c_void_p(t.data_ptr()), rows, cols, self._s()), self.h)
            self.stream.synchronize()
        return self

    def set_norm_stats(self, mean_hml, std_hml, mean_ih, std_ih):
        arr = np.concatenate([np.asarray(a, dtype=np.float32).reshape(262) for a in (mean_hml, std_hml, mean_ih, std_ih)])
        arr = np.ascontiguousarray(arr)
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_set_norm_stats(self.h, arr.ctypes.data_as(C.c_void_p)), self.h)
        return self

    def prepare(self):
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_prepare(self.h), self.h)
        return self

    # ---- schedule ---------------------------------------------------------------------------------
    def set_schedule(self, sampling_strategy="ddim50", beta_scheduler="cosine", diffusion_steps=1000):
        sch = make_schedule(beta_scheduler, diffusion_steps, sampling_strategy)
        tmap = np.ascontiguousarray(np.array(sch.timestep_map, dtype=np.int32))
        coef = np.ascontiguousarray(sch.device_coefficients())
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_set_schedule(self.h, tmap.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p), sch.num_timesteps, self._s()), self.h)
        self.schedule = sch
        self._strategy = sch.key()
        self.eta = 0.0
        return sch

    def use_schedule(self, sch):
        """The handle on the schedule OBJECT `sch` (a facade builds a new one per call), compared by CONTENT: the tables are uploaded, the time-embedding
        tables rebuilt and eta reset to 0 only when sch.key() differs from what the handle holds, so that nothing is re-captured through the (B, T, S)
        graph cache.  (The upload is set_schedule's, which is left as it stands: see DESIGN.md section 9g.)"""
        if self._strategy != sch.key():
            tmap = np.ascontiguousarray(np.array(sch.timestep_map, dtype=np.int32))
            coef = np.ascontiguousarray(sch.device_coefficients())
            with torch.cuda.device(self.device):
                check(self.lib.mmdm_set_schedule(self.h, tmap.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p), sch.num_timesteps, self._s()), self.h)
            self.schedule, self._strategy = sch, sch.key()
            self.eta = 0.0                                 # the upload resets the handle's eta table
        return sch

    def set_eta(self, eta):
        """mmdm_set_eta: the stochastic DDIM family (gaussian_diffusion.py:1939-1963), eta = 1 being DDPM-like.  Call after set_schedule (which resets
        it to 0).  While eta > 0 every begin / sample names a noise source (noise= or seed=); eta = 0 clears the table."""
        eta = float(eta)
        if eta < 0:
            raise ValueError(f"set_eta: eta={eta} must be >= 0")
        with torch.cuda.device(self.device):
            if eta == 0.0:
                check(self.lib.mmdm_set_eta(self.h, None, 0), self.h)
            else:
                tab = np.ascontiguousarray(self.schedule.eta_coefficients(eta))
                check(self.lib.mmdm_set_eta(self.h, tab.ctypes.data_as(C.c_void_p), self.schedule.num_timesteps), self.h)
        self.eta = eta
        return self

    def set_dual_weights(self, func, value):
        """Composition weight of ClassifierFreeSampleDualMDM (cfg_sampler.py:113-125) evaluated in float64 on the model-side
        timestep of every respaced step, exactly as the reference's lambdas do, then handed over as a float32 table."""
        t = np.asarray(self.schedule.timestep_map, dtype=np.int64)
        if func == "exp":
            w = np.exp(-value * (1000 - t))
        elif func == "exp-inv":
            w = 1 - np.exp(-value * (1000 - t))
        elif func == "lin":
            w = 1 - ((1000 - t) / 1000)
        elif func == "const":
            w = np.full(t.shape, value, dtype=np.float64)
        else:
            raise ValueError("Unknown function")
        w = np.ascontiguousarray(w.astype(np.float32))
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_set_dual_weights(self.h, w.ctypes.data_as(C.c_void_p), len(w)), self.h)
        return w

    # ---- key-padding mask ---------------------------------------------------------------------------
    def set_key_mask(self, valid):
        """mmdm_set_key_mask: valid [rows, T] (bool / 0-1; True = the frame exists) or None to clear.  Stays in force for module_forward and
        begin / run until cleared or replaced; rows = the call's n for module_forward 0, 1, 2, and B for module_forward 4 and the loop.
        precision "fp32" and "fp32_split" handles take a mask (the masked fp32 and two-plane attention kernels); "bf16" / "bf16_fp8", an MDM
        denoiser 1 and single_only 2 / 3 are refused by the library by name."""
        with torch.cuda.device(self.device):
            if valid is None:
                check(self.lib.mmdm_set_key_mask(self.h, None, 0, 0), self.h)
                self._reverse_mask = False
                return self
            v = np.ascontiguousarray((torch.as_tensor(valid).detach().cpu().numpy() != 0).astype(np.uint8))
            if v.ndim != 2:
                raise ValueError(f"set_key_mask: [rows, T] expected, got {v.shape}")
            check(self.lib.mmdm_set_key_mask(self.h, v.ctypes.data_as(C.c_void_p), v.shape[0], v.shape[1]), self.h)
        self._reverse_mask = True                # (begin_reverse refuses a masked handle by name)
        return self

    # ---- sampling ---------------------------------------------------------------------------------
    def _check_cond(self, who, cond):
        """cfg_form 1 / 2: the handle reads 3 / 5 text slices per cond row -- a narrower tensor would be read past its end"""
        k = {1: 3, 2: 5}.get(self.cfg.cfg_form)
        if k is not None and (cond.dim() != 2 or cond.shape[1] != k * self.cfg.text_dim):
            raise ValueError(f"{who}: cfg_form={self.cfg.cfg_form} takes cond [B, {k} * text_dim = {k * self.cfg.text_dim}], got {tuple(cond.shape)}")

    def begin(self, cond, x_T, *, noise=None, seed=None, x_start=None, init_image=None, skip_timesteps=0):
        """mmdm_begin, or mmdm_begin_opts when a keyword is given (the other arguments of MixerDiffusion.ddim_sample_loop; two-chain sampler and single_only=4):
        noise [n >= S - skip, B, T, 524] = the step noises by loop position, or seed = the device generator's (ops.randn(seed, k, B, T) is step k's
        noise) -- one of them while eta > 0 (set_eta); x_start [B, T' >= T, 524] pins the roots' ground path at every step; init_image [B, T, 524] /
        skip_timesteps start the chains from q_sample(init_image, S - 1 - skip, x_T) (skip > 0 and no image: zeros) and run the steps from there."""
        cond = cond.to(self.device, torch.float32).contiguous()
        x_T = x_T.to(self.device, torch.float32).contiguous()
        self._check_cond("begin", cond)
        B, T = x_T.shape[:2]
        S = self.schedule.num_timesteps
        skip = int(skip_timesteps)
        keep = [cond, x_T]
        opts = None
        if noise is not None or seed is not None or x_start is not None or init_image is not None or skip:
            if noise is not None and seed is not None:
                raise ValueError("begin: give the step noise as a buffer (noise=) or as a seed (seed=), not both")
            opts = BeginOptions()
            dev32 = lambda t: t.to(self.device, torch.float32).contiguous()
            if noise is not None:
                noise = dev32(noise)
                if noise.dim() != 4 or tuple(noise.shape[1:]) != (B, T, 524):
                    raise ValueError(f"begin: noise [steps, {B}, {T}, 524] expected, got {tuple(noise.shape)}")
                opts.noise_source, opts.noise, opts.noise_steps = 1, noise.data_ptr(), noise.shape[0]
                keep.append(noise)
            elif seed is not None:
                opts.noise_source, opts.seed = 2, int(seed) & 0xFFFFFFFFFFFFFFFF
            if x_start is not None:
                x_start = dev32(x_start)
                if x_start.dim() != 3 or x_start.shape[0] != B or x_start.shape[2] != 524:
                    raise ValueError(f"begin: x_start [{B}, T' >= {T}, 524] expected, got {tuple(x_start.shape)}")
                opts.x_start, opts.x_start_frames = x_start.data_ptr(), x_start.shape[1]
                keep.append(x_start)
            if init_image is not None:
                init_image = dev32(init_image)
                if tuple(init_image.shape) != (B, T, 524):
                    raise ValueError(f"begin: init_image [{B}, {T}, 524] expected, got {tuple(init_image.shape)}")
                opts.init_image = init_image.data_ptr()
                keep.append(init_image)
            opts.skip_timesteps = skip
            if (init_image is not None or skip) and 0 <= skip < S:
                a, b = self.schedule.q_sample_coefficients(S - 1 - skip)
                opts.init_coef[0], opts.init_coef[1] = float(a), float(b)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        # the copies into the handle run on the sampler's stream, possibly long after this call returns (several calls in flight):
        # keep the allocator from handing the inputs' memory out again before that stream has passed this point
        for t in keep:
            t.record_stream(self.stream)
        with torch.cuda.device(self.device):
            if opts is None:
                check(self.lib.mmdm_begin(self.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x_T.data_ptr()), B, T, self._s()), self.h)
            else:
                check(self.lib.mmdm_begin_opts(self.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x_T.data_ptr()), B, T, C.byref(opts), self._s()), self.h)
        self._keep = tuple(keep)
        self.B, self.T = B, T
        self.lens, self.rows = None, B * T
        self._hist = None
        self._left = S - skip
        self._steps = S - skip
        return self

    def begin_ragged(self, cond, x_T, lens, *, noise=None, seeds=None, noise_rows=None, x_start=None, init_image=None, skip_timesteps=0):
        """Begin a RAGGED call (mmdm_begin_ragged): B items of different lengths in one batch.  cond [B, .]; lens: B ints; x_T: the items' frames
        back to back [sum(lens), C], or a list of B tensors [T_i, C].  Every item's result is bit-identical to sampling it alone.
        With a keyword (mmdm_begin_ragged_opts; two-chain sampler and single_only=4; forms and shapes: pack_ragged_options) the same holds with begin()'s options: item b of
        seeds=[...] equals sample(cond[b:b+1], x_b[None], seed=seeds[b], ...), and seeds=ONE int makes a batch of equal lengths equal to sample(cond, x,
        seed=seed) of the uniform batch; noise / x_start / init_image are each item's own, packed or as lists."""
        lens = [int(v) for v in lens]
        ro = None
        if noise is not None or seeds is not None or noise_rows is not None or x_start is not None or init_image is not None or skip_timesteps:
            ro = pack_ragged_options(lens, noise=noise, seeds=seeds, noise_rows=noise_rows, x_start=x_start, init_image=init_image, skip_timesteps=skip_timesteps)
        if isinstance(x_T, (list, tuple)):
            x_T = torch.cat([t.to(self.device, torch.float32).reshape(-1, t.shape[-1]) for t in x_T], 0)
        cond = cond.to(self.device, torch.float32).contiguous()
        x_T = x_T.to(self.device, torch.float32).contiguous()
        B = len(lens)
        self._check_cond("begin_ragged", cond)
        if cond.shape[0] != B or x_T.dim() != 2 or x_T.shape[0] != sum(lens):
            raise ValueError(f"begin_ragged: cond rows {cond.shape[0]}, x_T {tuple(x_T.shape)} do not match {B} items of {sum(lens)} frames in all")
        keep = [cond, x_T]
        S, skip = self.schedule.num_timesteps, 0
        opts = host = None
        if ro is not None:
            opts, skip = BeginRaggedOptions(), ro["skip_timesteps"]
            for nm in ("noise", "x_start", "init_image"):
                if ro[nm] is not None:
                    t = ro[nm].to(self.device, torch.float32).contiguous()
                    setattr(opts, nm, t.data_ptr())
                    keep.append(t)
            if ro["noise"] is not None:
                opts.noise_source, opts.noise_steps = 1, ro["noise"].shape[0]
            elif ro["seeds"] is not None:
                host = ((C.c_ulonglong * B)(*ro["seeds"]), (C.c_int * B)(*ro["noise_rows"]))       # consumed before the call returns
                opts.noise_source = 2
                opts.item_seed, opts.item_noise_row = C.addressof(host[0]), C.addressof(host[1])
            opts.skip_timesteps = skip
            if (ro["init_image"] is not None or skip) and 0 <= skip < S:
                a, b = self.schedule.q_sample_coefficients(S - 1 - skip)
                opts.init_coef[0], opts.init_coef[1] = float(a), float(b)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for t in keep:
            t.record_stream(self.stream)
        arr = (C.c_int * B)(*lens)
        with torch.cuda.device(self.device):
            if opts is None:
                check(self.lib.mmdm_begin_ragged(self.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x_T.data_ptr()), B, arr, self._s()), self.h)
            else:
                check(self.lib.mmdm_begin_ragged_opts(self.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x_T.data_ptr()), B, arr, C.byref(opts), self._s()), self.h)
        rows, real, rag = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.mmdm_call_rows(self.h, C.byref(rows), C.byref(real), C.byref(rag)), self.h)
        self._keep = tuple(keep)
        self.B, self.T = B, max(lens)
        self.lens, self.rows = lens, rows.value
        self._hist = None
        self._left = self._steps = S - skip
        return self

    # ---- DDIM inversion (one-chain samplers) ------------------------------------------------------------
    def _reverse_refusals(self, who):
        """The sampler modes an inversion covers, refused by name otherwise with the status of MMDM_ERR_UNSUPPORTED / MMDM_ERR_STATE."""
        so = self.single_only
        if so == 0:
            raise MMDMError(f"[mmdm status 4] {who}: the two-chain MixerMDM sampler (single_only = 0) has no reverse step: MixerDiffusion overrides the step "
                            "and the reference gives it no reverse form", 4)
        if so in (2, 3):
            raise MMDMError(f"[mmdm status 4] {who}: single_only = {so} is superseded by single_only = 4 with cfg_form = {so - 1}, which takes the reverse step", 4)
        if getattr(self, "_reverse_mask", False):
            raise MMDMError(f"[mmdm status 4] {who}: a key mask is set on the handle; the reverse step takes none (clear it with set_key_mask(None))", 4)
        if getattr(self, "eta", 0.0):
            raise MMDMError(f"[mmdm status 2] {who}: eta is set on the handle; the reverse ODE is the deterministic path only (set_eta(0) clears it)", 2)

    def _reverse_start(self, lens):
        """Takes over the begun forward call: the motion is in the handle's x; the tables and the row map of the reverse update go to the device."""
        sch = self.schedule
        key = (sch.key(), str(self.device))
        if getattr(self, "_rev_key", None) != key:
            self._rev_coef = torch.from_numpy(np.ascontiguousarray(sch.device_coefficients())).to(self.device)
            self._rev_tab = torch.from_numpy(np.ascontiguousarray(sch.reverse_coefficients())).to(self.device)
            self._rev_idx = torch.arange(sch.num_timesteps, dtype=torch.int32, device=self.device)
            self._rev_key = key
        item = None
        if lens is not None:                     # frame row -> item, -1 for the group's padding rows (they stay zero)
            m = np.full(self.rows, -1, dtype=np.int32)
            m[:sum(lens)] = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
            item = torch.from_numpy(m).to(self.device)
        st = self.state(sync=False)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self._rev_x = st["x"].clone()
        for t in (self._rev_coef, self._rev_tab, self._rev_idx, item):
            if t is not None:
                t.record_stream(self.stream)
        self._rev_item, self._rev_pos = item, 0
        return self

    def begin_reverse(self, cond, x_0):
        """Begin a DDIM inversion of the motion x_0 [B, T, C] (GaussianDiffusion.ddim_reverse_sample, gaussian_diffusion.py:908-944; the one-chain samplers:
        single_only 1 / 4).  run_reverse() then takes reverse steps from respaced step 0 upwards; state()["x"] is the latent, state()["pred_xstart"] the
        last step's x0."""
        self._reverse_refusals("begin_reverse")
        self.begin(cond, x_0)
        return self._reverse_start(None)

    def begin_reverse_ragged(self, cond, x_0, lens):
        """begin_reverse for B motions of different lengths (begin_ragged's layout).  Every item's latent is bit-identical to inverting it alone."""
        self._reverse_refusals("begin_reverse_ragged")
        self.begin_ragged(cond, x_0, lens)
        return self._reverse_start(self.lens)

    def run_reverse(self, nsteps=None, use_graph=True):
        """nsteps reverse steps (None: those that are left, S - position).  The step at respaced index i: the forward step at i on the handle gives the model's
        x0 under the guidance wrapper (pred_xstart; its own update of x is discarded), mmdm_ddim_reverse_f32 takes x from the level of alphas_cumprod[i] to
        that of alphas_cumprod[i + 1], and x is written back.  Everything is queued on the sampler's stream; no host synchronisation."""
        if getattr(self, "_rev_x", None) is None:
            raise MMDMError("[mmdm status 2] run_reverse: call begin_reverse / begin_reverse_ragged first", 2)
        S, i0 = self.schedule.num_timesteps, self._rev_pos
        n = S - i0 if nsteps is None else int(nsteps)
        if n < 0 or n > S - i0:
            raise MMDMError(f"[mmdm status 1] run_reverse: {n} reverse steps requested, {S - i0} left in the schedule", 1)
        x = self._rev_x
        C_ = x.shape[-1]
        rows = x.numel() // C_
        for i in range(i0, i0 + n):
            self.seek(i)
            self.run(1, use_graph)
            st = self.state(sync=False)
            with torch.cuda.device(self.device):
                check(self.lib.mmdm_ddim_reverse_f32(C.c_void_p(st["pred_xstart"].data_ptr()), C.c_void_p(self._rev_coef.data_ptr()),
                                                     C.c_void_p(self._rev_tab.data_ptr()), S, C.c_void_p(self._rev_idx.data_ptr() + 4 * i),
                                                     C.c_void_p(x.data_ptr()), rows, C_,
                                                     C.c_void_p(self._rev_item.data_ptr()) if self._rev_item is not None else None, self._s()))
            with torch.cuda.stream(self.stream):
                st["x"].copy_(x)
        self._rev_pos = i0 + n
        return self

    def invert(self, cond, x_0, steps=None, use_graph=True):
        """DDIM inversion (ddim_reverse_sample driven `for i in range(steps)`, clip_denoised=False): the latent [B, T, C] at the level of respaced step
        `steps` (None = S: the ab_next = 0 level, the x_T of a plain sample).  For steps = k < S, sample_from(cond, latent, k) walks the same levels down
        again and ends the loop."""
        k = invert_steps(steps, self.schedule.num_timesteps)
        self.begin_reverse(cond, x_0)
        self.run_reverse(k, use_graph)
        lat = self.state()["x"].clone()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return lat

    def invert_ragged(self, cond, x_0, lens, steps=None, use_graph=True):
        """invert for a ragged batch: list of B latents [T_i, C], each bit-identical to invert(cond[b:b+1], x_b[None], steps)[0]."""
        k = invert_steps(steps, self.schedule.num_timesteps)
        self.begin_reverse_ragged(cond, x_0, lens)
        self.run_reverse(k, use_graph)
        lat = self.state()["x"][:sum(self.lens)].clone()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return [lat[o:o + t] for o, t in self.item_slices()]

    def sample_from(self, cond, x_k, start_step, use_graph=True, *, eta=None, **opts):
        """sample() of a chain that stands at respaced step `start_step`: x_k is its state there (a partial inversion: invert(steps=start_step)) and the loop
        runs the start_step + 1 steps start_step .. 0 -- begin followed by seek.  start_step = S - 1 is sample().  eta and the keywords are sample()'s;
        init_image / skip_timesteps are refused (they name the first step themselves)."""
        k = check_start_step(start_step, self.schedule.num_timesteps, init_image=opts.get("init_image"), skip_timesteps=opts.get("skip_timesteps", 0))
        if eta is not None and float(eta) != getattr(self, "eta", 0.0):
            self.set_eta(eta)
        self.begin(cond, x_k, **opts)
        self.seek(k)
        self.run(None, use_graph)
        st = self.state()
        res = st["pred_xstart"] if self.single_only else st["pred_xstart2"]
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return res.clone()

    def sample_ragged_from(self, cond, x_k, lens, start_step, use_graph=True, *, eta=None, **opts):
        """sample_from for a ragged batch: list of B results [T_i, C]."""
        k = check_start_step(start_step, self.schedule.num_timesteps, init_image=opts.get("init_image"), skip_timesteps=opts.get("skip_timesteps", 0))
        if eta is not None and float(eta) != getattr(self, "eta", 0.0):
            self.set_eta(eta)
        self.begin_ragged(cond, x_k, lens, **opts)
        self.seek(k)
        self.run(None, use_graph)
        st = self.state()
        res = (st["pred_xstart"] if self.single_only else st["pred_xstart2"])[:sum(self.lens)].clone()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return [res[o:o + t] for o, t in self.item_slices()]

    def item_slices(self):
        """(first row, length) of every item inside a group of a ragged call's buffers."""
        out, o = [], 0
        for t in self.lens:
            out.append((o, t))
            o += t
        return out

    def set_history(self, names=("influence_i1", "influence_i2", "out1", "out2", "out_influenced"), every=1):
        """Allocate history buffers [slots, 2B, T, C] for the requested side outputs (mixermdm.py:794-796, 805-808).  C = 524 for
        out1 / out2 / out_influenced; for the influences 262 in mixing modes 3-4 and 1 in modes 1-2 (the reference's shapes).
        Ragged call: [slots, 2, rows, C] -- cond half, uncond half, each a group of the call's frame rows (item_slices()).  A call begun with
        skip_timesteps executes S - skip steps and keeps as many entries, as the reference does."""
        S = getattr(self, "_steps", None) or self.schedule.num_timesteps
        slots = (S + every - 1) // every
        n = 2 * self.B
        bufs = {}
        rag = getattr(self, "lens", None) is not None
        for nm in ("influence_i1", "influence_i2", "out1", "out2", "out_influenced"):
            if nm in names:
                Cc = (262 if self.cfg.mixing_mode >= 3 else 1) if nm.startswith("influence") else 524
                bufs[nm] = torch.empty((slots, 2, self.rows, Cc) if rag else (slots, n, self.T, Cc), device=self.device, dtype=torch.float32)
        for b in bufs.values():
            b.record_stream(self.stream)
        ptr = lambda nm: C.c_void_p(bufs[nm].data_ptr() if nm in bufs else 0)
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_set_history(self.h, ptr("influence_i1"), ptr("influence_i2"), ptr("out1"), ptr("out2"), ptr("out_influenced"), every), self.h)
        self._hist = bufs
        return bufs

    def run(self, nsteps=None, use_graph=True):
        """nsteps=None: the steps that are left (all S after a plain begin; S - skip_timesteps after a begin that skips; step_index + 1 after seek)."""
        if nsteps is None:
            left = getattr(self, "_left", None)
            nsteps = self.schedule.num_timesteps if left is None else left
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_run(self.h, nsteps, int(use_graph), self._s()), self.h)
        if getattr(self, "_left", None) is not None:
            self._left -= nsteps
        return self

    def seek(self, step_index):
        """Continue the begun call from respaced step `step_index` (S-1 = first, 0 = last) with the chains as they stand."""
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_seek(self.h, int(step_index), self._s()), self.h)
        self._left = int(step_index) + 1
        return self

    def synchronize(self):
        self.stream.synchronize()

    def state(self, sync=True):
        """Views (no copy) of the handle's x, x2, pred_xstart, pred_xstart2, model_out -- after the queued work completes (sync=True), or
        at once for use ON the sampler's stream (sync=False: sample_async)."""
        ptrs = [C.c_void_p() for _ in range(5)]
        check(self.lib.mmdm_get_state(self.h, *[C.byref(p) for p in ptrs]), self.h)
        if sync:
            self.stream.synchronize()
        Cc = 262 if self.single_only == 1 else 524
        shape = (self.rows, Cc) if getattr(self, "lens", None) is not None else (self.B, self.T, Cc)      # ragged: the group's frame rows (first sum(lens) real)
        out = {}
        for nm, p in zip(("x", "x2", "pred_xstart", "pred_xstart2", "model_out"), ptrs):
            out[nm] = _from_ptr(p.value, shape, self.device) if p.value else None
        return out

    def sample(self, cond, x_T, use_graph=True, history=None, history_every=1, *, eta=None, noise=None, seed=None, x_start=None, init_image=None,
               skip_timesteps=0):
        """Full loop: MixerDiffusion.ddim_sample_loop (gaussian_diffusion.py:1769-1820) -> last pred_xstart2 (or pred_xstart, single).
        eta: None = as set_eta left it; a number = set_eta(eta) first (it stays set).  The other keywords are begin()'s."""
        if eta is not None and float(eta) != getattr(self, "eta", 0.0):
            self.set_eta(eta)
        self.begin(cond, x_T, noise=noise, seed=seed, x_start=x_start, init_image=init_image, skip_timesteps=skip_timesteps)
        hist = self.set_history(history, history_every) if history else None
        self.run(None, use_graph)
        st = self.state()
        res = st["pred_xstart"] if self.single_only else st["pred_xstart2"]
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return (res.clone(), hist) if history else res.clone()

    def sample_async(self, cond, x_T, use_graph=True, history=None, history_every=1):
        """sample() without a host synchronisation: the whole loop and the copy of its result are queued on the sampler's stream and the call
        returns at once -> (result tensor, history buffers or None, event recorded behind them).  Wait for the event (or synchronise the
        stream) before reading either from the host or another stream.  Several shared samplers (share()) driven this way overlap."""
        self.begin(cond, x_T)
        hist = self.set_history(history, history_every) if history else None
        self.run(None, use_graph)
        st = self.state(sync=False)
        with torch.cuda.stream(self.stream):
            res = (st["pred_xstart"] if self.single_only else st["pred_xstart2"]).clone()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return res, hist, ev

    def enqueue(self, cond, x_T, out, hist=None, history_every=1, use_graph=True):
        """A whole uniform sampling call through the C ABI ONLY (mmdm_begin, mmdm_set_history, mmdm_run, mmdm_copy_result on the sampler's
        stream): no tensor is created, no torch stream or allocator call is made -- safe to call from a worker thread while other threads
        capture step graphs (the caching allocator's event queries are not allowed beside a capture).  Everything is the caller's: cond
        [B, .] and x_T [B, T, C] contiguous fp32 on the device and ordered before the sampler's stream, `out` [B, T, C] preallocated, `hist`
        {name: preallocated [slots, 2B, T, C] buffer}; all must stay alive until the stream has passed the call."""
        B, T = x_T.shape[:2]
        h = hist or {}
        ptr = lambda nm: C.c_void_p(h[nm].data_ptr() if nm in h else 0)
        # the C side launches on whatever device is current: select the handle's (torch.cuda.device is a hipSetDevice pair, no allocator call)
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_begin(self.h, C.c_void_p(cond.data_ptr()), C.c_void_p(x_T.data_ptr()), B, T, self._s()), self.h)
            if h:
                check(self.lib.mmdm_set_history(self.h, ptr("influence_i1"), ptr("influence_i2"), ptr("out1"), ptr("out2"), ptr("out_influenced"), history_every), self.h)
            check(self.lib.mmdm_run(self.h, self.schedule.num_timesteps, int(use_graph), self._s()), self.h)
            check(self.lib.mmdm_copy_result(self.h, C.c_void_p(out.data_ptr()), self._s()), self.h)
        self.B, self.T, self.lens, self.rows = B, T, None, B * T
        self._left, self._steps = 0, self.schedule.num_timesteps

    def sample_ragged_async(self, cond, x_T, lens, use_graph=True, history=None, history_every=1, *, eta=None, **opts):
        """A whole ragged sampling call queued on the sampler's stream (no host synchronisation): -> (list of per-item results [T_i, C], history
        buffers [slots, 2, rows, C] or None, event).  Wait for the event before reading from the host or another stream.
        eta as in sample(); the other keywords are begin_ragged()'s."""
        if eta is not None and float(eta) != getattr(self, "eta", 0.0):
            self.set_eta(eta)
        self.begin_ragged(cond, x_T, lens, **opts)
        hist = self.set_history(history, history_every) if history else None
        self.run(None, use_graph)
        st = self.state(sync=False)
        with torch.cuda.stream(self.stream):
            res = (st["pred_xstart"] if self.single_only else st["pred_xstart2"])[:sum(self.lens)].clone()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return [res[o:o + t] for o, t in self.item_slices()], hist, ev

    def sample_ragged(self, cond, x_T, lens, use_graph=True, *, eta=None, **opts):
        """Ragged MixerDiffusion.ddim_sample_loop: list of B results [T_i, C].  eta and the options: sample_ragged_async."""
        items, _, ev = self.sample_ragged_async(cond, x_T, lens, use_graph, eta=eta, **opts)
        ev.synchronize()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return items

    # ---- teacher-forced module forwards (tests / swappable inner protocol) ----------------------------
    def module_forward(self, which, x, cond, t, x2=None):
        """which: 0 denoiser1, 1 denoiser2, 2 Mixer.forward, 3 denoiser1 in "dual_individual" mode (inputs are the CFG-doubled batch);
        4 ClassifierFreeSampleModelX2.forward (B un-doubled rows in, B combined rows out).  The schedule survives; a begun call does not."""
        x = x.to(self.device, torch.float32).contiguous()
        cond = cond.to(self.device, torch.float32).contiguous()
        x2c = x2.to(self.device, torch.float32).contiguous() if x2 is not None else None
        n, T = x.shape[:2]
        out = torch.empty(n, T, 262 if which == 0 else 524, device=self.device, dtype=torch.float32)   # which 1 with single_only=2: n = 4B rows; 3 = dual_individual
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device):
            check(self.lib.mmdm_module_forward(self.h, which, C.c_void_p(x.data_ptr()), C.c_void_p(x2c.data_ptr() if x2c is not None else 0),
                                               C.c_void_p(cond.data_ptr()), int(t), C.c_void_p(out.data_ptr()), n, T, self._s()), self.h)
        self.stream.synchronize()
        return out

    def graph_stats(self):
        """(steps captured, steps replayed, graphs cached) of the handle's hipGraph cache.  Its key is everything a captured step bakes in: B, T and
        the schedule's S; whether a key mask is set, the call's noise form and whether it pins x_start; for a ragged call the group stride in rows and
        the query tiles of the longest item instead of T -- with MDM as denoiser 1 the token stride and token tiles as well (csrc/mmdm.hip GraphKey)."""
        cap, rep, n = C.c_int64(), C.c_int64(), C.c_int()
        check(self.lib.mmdm_graph_stats(self.h, C.byref(cap), C.byref(rep), C.byref(n)), self.h)
        return cap.value, rep.value, n.value

    def graphs_parked(self):
        """Graph execs of the PROCESS kept past their cache entry's life (mmdm_graph_parked: include/mmdm.h, mmdm_create_shared)."""
        return int(self.lib.mmdm_graph_parked())

    # ---- profiling ----------------------------------------------------------------------------------
    def profile(self, on=True):
        check(self.lib.mmdm_profile_enable(self.h, int(on)), self.h)

    def profile_read(self, which):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(self.lib.mmdm_profile_read(self.h, which, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), self.h)
        return ms.value, n.value, fl.value, by.value


def _from_ptr(ptr, shape, device):
    """Wrap a device pointer owned by the handle as a torch tensor (no copy) via __cuda_array_interface__."""
    class _Holder:
        pass
    hld = _Holder()
    hld.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 3, "strides": None}
    return torch.as_tensor(hld, device=device)
