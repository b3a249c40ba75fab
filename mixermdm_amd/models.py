"""Host-side mirror of the reference's `src/models` operator API for the denoising path, backed by libmmdm_hip.so.

Reference surface mirrored:
  * ``MixerMDM(cfg, num_frames=300, sampling_strategy="ddim50", store_influence=True, align=True)`` with
    ``forward(batch)`` / ``forward_test(batch)`` / ``load_state_dict`` and the knobs ``.mixing.mode``,
    ``.mixing.force_influence_val``, ``.mixing_mode``, ``.sampling_strategy``, ``.cfg_mixing_weight``
    (src/models/mixermdm.py:18-19, 490-602);
  * the inner callables: ``Mixer(x1, timesteps, cond, mask, x2)`` (mixermdm.py:660), denoisers
    ``f(x, timesteps, cond=, mask=)`` (in2in.py:401), ``ClassifierFreeSampleModelX2`` (cfg_sampler.py:31-56) and
    ``MixerDiffusion.ddim_sample_loop`` (gaussian_diffusion.py:1769-1820).

Python only moves pointers: parameters live in torch tensors under the reference's state_dict key names and are copied
into the HIP handle's packed layout; every arithmetic op of the loop is a HIP kernel.  Text encoding (CLIP tower +
clipTransEncoder, mixermdm.py:283-356) is upstream of this path: pass ``batch["cond"]`` ([B, 8*768], layout
mixermdm.py:342-354) or register ``text_encoder``.
"""
import os
import numpy as np
import torch
from torch import nn

from .configs import get_config
from .sampler import Sampler, pe_table
from .schedule import get_named_beta_schedule, space_timesteps, RespacedSchedule
from .synthetic import mixer_shapes, synthetic_state_dict, synthetic_stats

# state_dict prefixes of the reference's MixerMDM that are NOT on the denoising path (CLIP tower, sub-model facades,
# training-only discriminators); accepted and ignored by load_state_dict.
OFF_PATH_PREFIXES = ("model1.", "model2.", "denoiser1.", "denoiser2.", "discriminator_i.", "discriminator_I.", "clipTransEncoder.", "clip_ln.",
                     "token_embedding.", "clip_transformer.", "positional_embedding", "ln_final.")

HISTORY_BUDGET_BYTES = 32 << 30


def _holder_tree(root, name, tensor):
    """Register `tensor` as parameter `name` ("a.b.0.weight") on nested container modules so that state_dict() yields the
    reference's key names."""
    parts = name.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, nn.Module())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


def key_valid_of(mask):
    """The reference's `mask` argument (float [n, T, k]; only mask[..., 0] is used) -> bool [n, T], True = the frame exists
    (key_padding_mask = ~(mask[..., 0] > 0.5): in2in.py:411-436, influence.py:105-117)."""
    if mask.dim() != 3:
        raise ValueError(f"mask: [n, T, k] expected, got {tuple(mask.shape)}")
    return mask[..., 0] > 0.5


class _KeyMask:
    """Sets the key mask on a sampler's handle for the duration of one call and clears it afterwards (precision "fp32" and "fp32_split"
    handles); the cases the library refuses -- "bf16" / "bf16_fp8" handles, an MDM denoiser 1, single_only 2 / 3: MMDM_ERR_UNSUPPORTED from
    mmdm_set_key_mask or from the masked call itself -- raise NotImplementedError with the library's message.
    mask=None: nothing is touched."""
    UNSUPPORTED = 4

    def __init__(self, smp, mask):
        self.smp, self.mask = smp, mask

    def __enter__(self):
        if self.mask is not None:
            from ._lib import MMDMError
            try:
                self.smp.set_key_mask(key_valid_of(self.mask))
            except MMDMError as e:
                if e.status == self.UNSUPPORTED:
                    raise NotImplementedError(str(e)) from None
                raise
        return self.smp

    def __exit__(self, etype, exc, tb):
        if self.mask is not None:
            from ._lib import MMDMError
            self.smp.set_key_mask(None)
            if isinstance(exc, MMDMError) and exc.status == self.UNSUPPORTED:
                raise NotImplementedError(str(exc)) from None
        return False


class _Callable(nn.Module):
    """Base of the inner callables: shares the owner's sampler."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)

    @staticmethod
    def _uniform_t(timesteps):
        t = timesteps.reshape(-1)
        if not bool((t == t[0]).all()):
            raise NotImplementedError("the HIP path runs one timestep per call (the sampler always passes t = [i]*B: gaussian_diffusion.py:1872)")
        return int(t[0])


class DenoiserHandle(_Callable):
    """in2INDenoiser / InterDenoiser protocol: f(x [n,T,nf*k], timesteps [n], cond=[n,.], mask=None) -> [n,T,nf*k]."""

    def __init__(self, owner, which):
        super().__init__(owner)
        self.which = which
        self.text_dim = 768

    def forward(self, x, timesteps, mask=None, cond=None):
        n = x.shape[0]
        if n % 2:
            raise ValueError("the HIP denoiser works on the CFG-doubled batch (even number of rows)")
        smp = self._owner._sampler_for(n // 2, x.shape[1])
        with _KeyMask(smp, mask):
            return smp.module_forward(self.which, x, cond, self._uniform_t(timesteps))


class Mixer(_Callable):
    """Mixer.forward protocol (mixermdm.py:660): out_influenced for the CFG-doubled batch.  Holds the reference's knobs."""

    def __init__(self, owner, mixing_mode, store_influence, force_influence_val, mode="train", align=True):
        super().__init__(owner)
        self.mixing_mode = mixing_mode
        self.store_influence = store_influence
        self.force_influence_val = force_influence_val
        self.mode = mode
        self.align = align
        self.history_influence_i1, self.history_influence_i2 = [], []
        self.history_out1, self.history_out2, self.history_out_influenced = [], [], []

    def forward(self, x1, timesteps, cond=None, mask=None, x2=None):
        if self.mixing_mode not in (1, 2, 3, 4):
            raise ValueError("Mixing mode not recognized")
        smp = self._owner._sampler_for(x1.shape[0] // 2, x1.shape[1])
        with _KeyMask(smp, mask):
            return smp.module_forward(2, x1, cond, self._uniform_t(timesteps), x2=x2)


class ClassifierFreeSampleModelX2(nn.Module):
    """cfg_sampler.py:31-56.  Inside the sampling loop the doubling and the s*cond + (1-s)*uncond combine are part of the captured HIP
    step; called on its own (the reference's inner-callable protocol ``f(x, x2, timesteps, cond, mask)``, cfg_sampler.py:38) it runs the
    same kernels through ``mmdm_module_forward(which=4)``: B un-doubled rows in, B combined rows out."""

    def __init__(self, model, cfg_scale):
        super().__init__()
        self.model = model
        self.s = cfg_scale

    def forward(self, x, x2, timesteps, cond=None, mask=None):
        if cond is None:
            raise NotImplementedError("the HIP mixer is text-conditioned: cond [B, 8*768] is required (mixermdm.py:342-354)")
        mixer = self.model
        if mixer.mixing_mode not in (1, 2, 3, 4):
            raise ValueError("Mixing mode not recognized")
        owner = mixer._owner
        smp = owner._sampler_for(x.shape[0], x.shape[1], cfg_scale=self.s)
        with _KeyMask(smp, mask):             # B rows: the library repeats the mask for its own doubling (cfg_sampler.py:47-48)
            return smp.module_forward(4, x, cond, _Callable._uniform_t(timesteps), x2=x2)


class MixerDiffusion:
    """Two-chain DDIM sampler (gaussian_diffusion.py:1434-1463, 1769-1965): schedule tables on the host, loop on the GPU."""

    def __init__(self, use_timesteps, align=True, *, betas, **kwargs):
        self.align = align
        self.schedule = RespacedSchedule(betas, use_timesteps)
        self.timestep_map = self.schedule.timestep_map
        self.num_timesteps = self.schedule.num_timesteps
        self.original_num_steps = self.schedule.original_num_steps

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None, randomize_class=False,
                         cond_fn_with_grad=False, dump_steps=None, const_noise=False, x_start=None, *, step_noise=None, seed=None):
        """eta, skip_timesteps, init_image and x_start as in the reference (gaussian_diffusion.py:1854-1882, 1936-1965).  Two keyword-only arguments of
        this port name the noise of the eta > 0 steps: step_noise [>= S - skip, B, T, 524] (slot k = th.randn_like(x) of the k-th executed step) or
        seed (the device generator; ops.randn(seed, k, B, T) is slot k).  With eta > 0 and neither, a seed is drawn from torch's default generator:
        torch.manual_seed reproduces a run.  At eta = 0 the noise is multiplied by zero and neither is read."""
        if dump_steps is not None or const_noise:
            raise NotImplementedError()                                   # gaussian_diffusion.py:1794-1797
        if clip_denoised or denoised_fn is not None or cond_fn is not None or randomize_class or cond_fn_with_grad:
            raise NotImplementedError("HIP sampler implements the configuration MixerMDM.forward uses: clip_denoised=False, eta=0, no guidance fn")
        eta = float(eta)
        if eta < 0:
            raise ValueError(f"eta={eta} must be >= 0")
        if step_noise is not None and seed is not None:
            raise ValueError("give the step noise as a buffer (step_noise=) or as a seed (seed=), not both")
        if eta == 0.0:
            step_noise = seed = None
        elif step_noise is None and seed is None:
            seed = _draw_seed()
        opts = dict(eta=eta, noise=step_noise, seed=seed, x_start=x_start, init_image=init_image, skip_timesteps=int(skip_timesteps))
        mixer = model.model if isinstance(model, ClassifierFreeSampleModelX2) else model
        owner = mixer._owner
        model_kwargs = model_kwargs or {}
        mask = model_kwargs.get("mask")      # handed to the model unchanged at every step (gaussian_diffusion.py:1871-1899): set once on the handle
        cond = model_kwargs["cond"]
        B, T, _ = shape
        dev = owner.device
        x_T = noise if noise is not None else torch.randn(*shape, device=dev)
        return owner._run_loop(self, cond, x_T, cfg_scale=getattr(model, "s", owner.cfg_mixing_weight), mask=mask, opts=opts)


def _history_plan(mode, store_influence, keep_history, S, skip, history_every, mixing_mode):
    """The history side outputs of a MixerMDM call -> ({name: width} in the library's order, slots, bytes per (motion, frame)).  keep_history: None = what
    the mode says (store_influence -> the influences; "eval" -> out1 / out2 / out_influenced), False = none.  One slot per EXECUTED step, every
    history_every-th; modes 1-2 keep the un-expanded [2B, T, 1] influence (mixermdm.py:739-745); a frame has a cond and an uncond row of fp32."""
    names = []
    if keep_history is None or keep_history:
        if store_influence:
            names += ["influence_i1", "influence_i2"]
        if mode == "eval":
            names += ["out1", "out2", "out_influenced"]
    kept = {n: (262 if mixing_mode >= 3 else 1) if n.startswith("influence") else 524 for n in names}
    slots = (S - skip + history_every - 1) // history_every
    return kept, slots, slots * 2 * 4 * sum(kept.values())


class MixerMDM(nn.Module):
    def __init__(self, cfg, num_frames=300, sampling_strategy="ddim50", store_influence=True, align=True, config_root=None):
        super().__init__()
        self.cfg = cfg
        root = config_root or os.getcwd()
        self.cfg_model1 = get_config(os.path.join(root, cfg.MODEL1) if not os.path.isabs(cfg.MODEL1) else cfg.MODEL1)
        self.cfg_model2 = get_config(os.path.join(root, cfg.MODEL2) if not os.path.isabs(cfg.MODEL2) else cfg.MODEL2)
        if self.cfg_model1.NAME not in ("in2INind", "MDM"):
            raise NotImplementedError(f"MODEL1.NAME={self.cfg_model1.NAME}")
        if self.cfg_model2.NAME not in ("in2IN", "InterGen"):
            raise NotImplementedError(f"MODEL2.NAME={self.cfg_model2.NAME}")
        self.align = align
        self.store_influence = store_influence
        self.num_frames = num_frames
        g = cfg.GENERATOR if "GENERATOR" in cfg else cfg
        self.nfeats = g.INPUT_DIM
        c1, c2 = self.cfg_model1, self.cfg_model2
        # MODEL1 and MODEL2 are separate configs (mixermdm.py:32-40): denoiser1 carries its own sizes (d1_*), denoiser2 the d_* ones
        self.dims = dict(d_latent=c2.LATENT_DIM, d_ff=c2.FF_SIZE, d_layers=c2.NUM_LAYERS, m_latent=g.LATENT_DIM, m_ff=g.FF_SIZE, m_layers=g.NUM_LAYERS,
                         d1_latent=c1.LATENT_DIM, d1_ff=c1.FF_SIZE, d1_layers=c1.NUM_LAYERS)
        self.d_heads, self.d1_heads, self.m_heads = c2.NUM_HEADS, c1.NUM_HEADS, g.NUM_HEADS
        self.model1_kind = 1 if c1.NAME == "MDM" else 0
        self.cfg_mixing_weight = cfg.CFG_WEIGHT
        self.text_dim = 768
        self.mixing_mode = cfg.MIXING_MODE
        self.diffusion_steps = cfg.DIFFUSION_STEPS
        self.beta_scheduler = cfg.BETA_SCHEDULER
        self.sampling_strategy = sampling_strategy
        self.betas = get_named_beta_schedule(self.beta_scheduler, self.diffusion_steps)
        self.history_every = 1
        self.precision = "fp32"             # "fp32" (native fp32 MFMA, the parity path) | "fp32_split" (same accuracy, bf16 matrix cores) | "bf16"
                                            # (MODEL1.NAME == "MDM": "fp32" or "fp32_split"; the handle refuses the bf16 modes by name)
        self.text_encoder = None            # optional callable(batch) -> cond [B, 8*768] overriding the built-in text stage
        self._text_sd, self._text_enc = None, None
        self.mixing = Mixer(self, self.mixing_mode, store_influence, cfg.FORCE_INFLUENCE_VAL, align=align)
        self.mixing.add_module("denoiser1", DenoiserHandle(self, 0))
        if self.model1_kind == 1:
            # MDMDenoiser.text_dim is hard-coded to 256 (mdm.py:238) while its cond is added to the latent-sized timestep embedding
            # (mdm.py:279): the cond slice width is the latent size (they coincide for the reference's MDM, LATENT_DIM = 256).
            self.mixing.denoiser1.text_dim = c1.LATENT_DIM
        self.mixing.add_module("denoiser2", DenoiserHandle(self, 1))
        # the reference also exposes them as .denoiser1/.denoiser2 (mixermdm.py:67-68); plain attributes here, not re-registered
        object.__setattr__(self, "denoiser1", self.mixing.denoiser1)
        object.__setattr__(self, "denoiser2", self.mixing.denoiser2)
        # parameters under the reference's key names (mixing.*), zero-initialised until loaded
        self._model1 = "MDM" if self.model1_kind else "in2INind"
        for k, shp in mixer_shapes(mixing_mode=self.mixing_mode, model1=self._model1, **self.dims).items():
            _holder_tree(self, "mixing." + k, torch.zeros(shp))
        self._sampler = None
        self._dirty = True
        self._stats = None
        self._try_load_norm_stats()
        self._try_load_submodel_checkpoints()

    # ---- weights / stats -----------------------------------------------------------------------------
    def _try_load_norm_stats(self):
        """MotionNormalizerTorch{,HML3D}.__init__ paths (src/utils/utils.py:46-47, 66-67)."""
        paths = ["./data/HumanML3D/mean_ih_new.npy", "./data/HumanML3D/std_ih_new.npy", "./data/global_mean.npy", "./data/global_std.npy"]
        if all(os.path.exists(p) for p in paths):
            self.set_norm_stats(*[np.load(p) for p in paths])

    def _try_load_submodel_checkpoints(self):
        """The reference's constructor loads the two frozen sub-models from MODEL1/MODEL2.CHECKPOINT (mixermdm.py:43-59): raw state dicts
        for in2IN (keys ``decoder.net_{individual,interaction}.*``), ``{"state_dict": ...}`` with a Lightning ``model.`` prefix for MDM
        (denoiser under ``model.*``) and InterGen (``decoder.net.*``).  Here they are optional: when a file exists its denoiser weights
        initialise ``mixing.denoiser{1,2}.*`` (a MixerMDM checkpoint loaded afterwards carries the same tensors and overrides them)."""
        own = dict(self.named_parameters())
        for which, cfgm in (("1", self.cfg_model1), ("2", self.cfg_model2)):
            path = cfgm.CHECKPOINT if "CHECKPOINT" in cfgm else None
            if not path or not os.path.exists(path):
                continue
            ck = torch.load(path, map_location="cpu")
            if cfgm.NAME == "MDM":
                sd = {k[6:]: v for k, v in ck["state_dict"].items()}
                pfx = "model."
            elif cfgm.NAME == "InterGen":
                sd = {k.replace("model.", "") if "model" in k else k: v for k, v in ck["state_dict"].items()}
                pfx = "decoder.net."
            else:
                sd = ck
                pfx = "decoder.net_individual." if which == "1" else "decoder.net_interaction."
            with torch.no_grad():
                for k, v in sd.items():
                    if k.startswith(pfx):
                        tgt = "mixing.denoiser%s.%s" % (which, k[len(pfx):])
                        if tgt in own and tuple(own[tgt].shape) == tuple(v.shape):
                            own[tgt].copy_(v)
            self._dirty = True

    def set_norm_stats(self, mean_hml, std_hml, mean_ih, std_ih):
        self._stats = [np.asarray(a, dtype=np.float32).reshape(262) for a in (mean_hml, std_hml, mean_ih, std_ih)]
        self._dirty = True

    def init_synthetic(self, seed=0, std=0.02, bias_std=0.0, stats_seed=3):
        """Random-init weights of the reference architecture + synthetic normaliser stats (no checkpoints offline)."""
        sd = synthetic_state_dict(seed=seed, std=std, bias_std=bias_std, mixing_mode=self.mixing_mode, model1=self._model1, **self.dims)
        self.load_state_dict({"mixing." + k: v for k, v in sd.items()})
        st = synthetic_stats(stats_seed)
        self.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
        return self

    def load_state_dict(self, state_dict, strict=True):
        own = {k for k, _ in self.named_parameters()}
        mine, unexpected = {}, []
        for k, v in state_dict.items():
            if k in own:
                mine[k] = v
            elif k.endswith("sequence_pos_encoder.pe") or k.startswith(OFF_PATH_PREFIXES):
                continue                       # regenerated tables / off-path modules of the reference's checkpoint
            else:
                unexpected.append(k)
        missing = sorted(own - set(mine))
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for MixerMDM:\n\tMissing key(s): %s\n\tUnexpected key(s): %s" % (missing[:8], unexpected[:8]))
        params = dict(self.named_parameters())
        with torch.no_grad():
            for k, v in mine.items():
                if tuple(v.shape) != tuple(params[k].shape):
                    raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)}, the shape in current model is {tuple(params[k].shape)}")
                params[k].copy_(v)
        self._dirty = True
        # text-conditioning stage: when the checkpoint carries the CLIP tower and the three clipTransEncoder heads
        # (mixermdm.py:212-259), generate_cond runs on the GPU too; built lazily on the model's device
        need = ("token_embedding.weight", "positional_embedding", "ln_final.weight", "clipTransEncoder.layers.0.linear1.weight", "clip_ln.weight")
        if all(k in state_dict for k in need):
            pre = ("token_embedding.", "positional_embedding", "clip_transformer.", "ln_final.", "clipTransEncoder.", "clip_ln.",
                   "model1.clipTransEncoder", "model1.clip_ln", "model2.clipTransEncoder", "model2.clip_ln", "model1.clip_model.", "model1.embed_text.")
            self._text_sd = {k: v for k, v in state_dict.items() if k.startswith(pre)}
            self._text_enc = None
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def _apply(self, fn, recurse=True):
        self._dirty = True
        return super()._apply(fn, recurse)

    @property
    def device(self):
        return next(self.parameters()).device

    def _sampler_for(self, B, T, cfg_scale=None):
        if cfg_scale is not None and float(cfg_scale) != float(self.cfg_mixing_weight):
            self.cfg_mixing_weight = cfg_scale         # the guidance scale is a handle constant (fused into the blend kernel)
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("MixerMDM runs on an MI355X only: call .to('cuda:N') first (no CPU path)")
        m = self.mixing
        key = (str(dev), m.mixing_mode, bool(m.align), m.force_influence_val, self.cfg_model2.NAME, self.cfg_model1.NAME, self.precision,
               float(self.cfg_mixing_weight))
        s = self._sampler
        if s is None or s._key != key or B > s.cfg.max_batch or T > s.cfg.max_frames:
            if s is not None:
                s.close()
            s = Sampler(d_heads=self.d_heads, d1_heads=self.d1_heads, model1_kind=self.model1_kind, m_heads=self.m_heads,
                        mixing_mode=m.mixing_mode, align=m.align, xstart_align=True,
                        model2_kind=1 if self.cfg_model2.NAME == "InterGen" else 0, force_influence_val=m.force_influence_val,
                        cfg_scale=self.cfg_mixing_weight, max_batch=max(B, s.cfg.max_batch if s else 1),
                        max_frames=max(T, self.num_frames), device=dev, precision=self.precision, **self.dims)
            s._key = key
            self._sampler, self._dirty = s, True
        if self._dirty:
            if self._stats is None:
                raise RuntimeError("normaliser statistics missing: ./data/global_{mean,std}.npy and ./data/HumanML3D/{mean,std}_ih_new.npy "
                                   "not found (src/utils/utils.py:46-47,66-67); call set_norm_stats(...)")
            s.load_state_dict({k[len("mixing."):]: p.data for k, p in self.named_parameters()})
            s.set_norm_stats(*self._stats)
            s.prepare()
            s._strategy = None
            self._dirty = False
        return s

    # ---- conditioning -------------------------------------------------------------------------------
    def generate_cond(self, batch):
        if "cond" in batch:
            return batch["cond"]
        if self.text_encoder is None and getattr(self, "_text_sd", None) is not None:
            if self._text_enc is None or self._text_enc.tower.table.device != self.device:
                from .text import MixerTextEncoder
                heads = self._text_sd["clip_transformer.resblocks.0.attn.in_proj_weight"].shape[1] // 64 if "clip_transformer.resblocks.0.attn.in_proj_weight" in self._text_sd else 12
                self._text_enc = MixerTextEncoder(self._text_sd, clip_heads=heads, head_heads=8, device=self.device, model2=self.cfg_model2.NAME,
                                                  model1=self.cfg_model1.NAME)
            return self._text_enc.generate_cond(batch)
        if self.text_encoder is None:
            raise NotImplementedError("text encoding (CLIP ViT-L/14 tower + clipTransEncoder, mixermdm.py:283-356) is upstream of the HIP path: "
                                      "pass batch['cond'] [B, 8*768] or set model.text_encoder")
        return self.text_encoder(batch)

    # ---- sampling -----------------------------------------------------------------------------------
    def _run_loop(self, diffusion, cond, x_T, cfg_scale=None, mask=None, opts=None):
        B, T = x_T.shape[:2]
        smp = self._sampler_for(B, T, cfg_scale=cfg_scale)
        with _KeyMask(smp, mask):
            return self._run_loop_on(smp, diffusion, cond, x_T, opts)

    def _run_loop_on(self, smp, diffusion, cond, x_T, opts=None):
        B, T = x_T.shape[:2]
        sch = diffusion.schedule
        # the facade builds a new MixerDiffusion per call (as the reference does, mixermdm.py:515-522): compare schedules by CONTENT so
        # that the tables are uploaded, the time-embedding tables rebuilt and (through the (B, T, S) graph cache) nothing re-captured
        # only when the strategy really changed
        smp.use_schedule(sch)
        opts = dict(opts or {})
        eta = opts.pop("eta", 0.0)
        if eta != getattr(smp, "eta", 0.0):
            smp.set_eta(eta)
        skip = opts.get("skip_timesteps", 0)
        if not 0 <= skip < sch.num_timesteps:
            raise ValueError(f"skip_timesteps={skip} outside [0, {sch.num_timesteps})")
        m = self.mixing
        kept, _, per_row = _history_plan(m.mode, m.store_influence, None, sch.num_timesteps, skip, self.history_every, m.mixing_mode)
        names = list(kept)
        need = per_row * B * T
        if need > HISTORY_BUDGET_BYTES:
            raise MemoryError(f"history side outputs need {need / 2**30:.1f} GiB for {sch.num_timesteps} steps (the reference keeps every step: "
                              "mixermdm.py:794-808); set model.history_every = k to keep every k-th step, or store_influence=False / forward_test")
        try:
            smp.begin(cond, x_T, **opts)
            hist = smp.set_history(names, self.history_every) if names else {}
            smp.run(None, use_graph=True)
            out = smp.state()["pred_xstart2"].clone()
        finally:
            if eta:                                        # eta belongs to this call: the facade's other entry points find the handle as they left it
                smp.set_eta(0.0)
        torch.cuda.current_stream(smp.device).wait_stream(smp.stream)
        as_list = lambda n: list(hist[n].unbind(0)) if n in hist else []
        m.history_influence_i1, m.history_influence_i2 = as_list("influence_i1"), as_list("influence_i2")
        m.history_out1, m.history_out2, m.history_out_influenced = as_list("out1"), as_list("out2"), as_list("out_influenced")
        return out

    # ---- many calls at once: the reference's callers, redesigned --------------------------------------------------
    def _pool(self, k, B, T):
        """k samplers over ONE weight set: the facade's own handle plus k - 1 handles that borrow its weights (mmdm_create_shared), each with its
        own stream, workspace (B, T), schedule tables and graph cache."""
        main = self._sampler_for(B, T)
        pool = getattr(self, "_shared", None)
        if pool is None or pool["parent"] is not main or pool["B"] < B or pool["T"] < T:
            if pool is not None:
                for c in pool["kids"]:
                    c.close()
            pool = {"parent": main, "B": B, "T": T, "kids": []}
            self._shared = pool
        while len(pool["kids"]) < k - 1:
            pool["kids"].append(main.share(max_batch=B, max_frames=max(T, self.num_frames)))
        return [main] + pool["kids"][:k - 1]

    def sample_many(self, batches, mode="eval_intermediate", batching="ragged", inflight=2, max_rows=4800, max_items=64, keep_history=None, *,
                    eta=0.0, skip_timesteps=0):
        """Many sampling calls in one go -- what the reference's callers do one after the other: the inference script calls ``model(batch)`` ten
        times at B = 1 (src/scripts/infer/mixermdm.py:184-188), the evaluation datasets call ``forward_test`` once per item with that item's
        own length (src/evaluation/datasets.py:100-116).  `batches`: reference-style batch dicts (text lists or a precomputed 'cond' [b, 8*768];
        'motion_lens'[0] = T; optionally 'x_T' [b, T, 524]).  Returns one result dict per batch, as ``forward`` (mode="eval") /
        ``forward_test`` (mode="eval_intermediate") would -- every motion BIT-IDENTICAL to that call's on the same x_T.

        batching: "sequential" = the reference's loop (one call after the other on one handle);
                  "inflight"   = `inflight` handles over one weight set, calls dealt round-robin, each on its own stream.  Bit-identical, and
                                 measured worth 1.00-1.03 x (the GPU co-schedules two such streams hardly at all: LAB_NOTES.md round 5) --
                                 kept for callers whose requests arrive at different times, not as a throughput lever;
                  "ragged"     = the calls' motions packed into ragged batches of <= max_rows frames / <= max_items motions
                                 (mmdm_begin_ragged: per-sequence lengths as device data; GEMMs at the efficiency of a full batch).
        keep_history: None = what the mode says (store_influence -> influence lists; "eval" -> out1 / out2 / out_influenced), False = outputs only.

        The loop's other arguments (ddim_sample_loop's; "sequential" and "ragged", bitwise the same motions and histories either way): eta and
        skip_timesteps belong to the call; a batch dict may carry 'seed' (int) or 'step_noise' [>= S - skip, b, T, 524] (read at eta > 0 only; with
        neither, one seed per batch is drawn from torch's default generator, in batch order), 'x_start' [b, T' >= T, 524] and 'init_image' [b, T, 524].
        Motion j of a batch draws the noise of row j of that batch's call.  One noise form per call, and x_start / init_image for every batch or
        none (a step's kernel form belongs to the call): otherwise ValueError.  Histories hold S - skip_timesteps entries."""
        if batching not in ("sequential", "inflight", "ragged"):
            raise ValueError(f"batching {batching!r} not recognized")
        eta, skip = float(eta), int(skip_timesteps)
        if eta < 0:
            raise ValueError(f"eta={eta} must be >= 0")
        use_opts, form, seeds = _loop_forms(batches, eta, skip, "sample_many", no_opts='batching="inflight" takes no eta / skip_timesteps / x_start / init_image; '
                                            'use "ragged" or "sequential"' if batching == "inflight" else None)
        m = self.mixing
        m.mode = mode
        with torch.no_grad():
            conds = [self.generate_cond(b) for b in batches]
        Ts = [int(b["motion_lens"][0]) for b in batches]
        Bs = [int(c.shape[0]) for c in conds]
        dev = self.device
        xs = [b["x_T"].to(dev, torch.float32) if "x_T" in b else torch.randn(nb, T, self.nfeats * 2, device=dev) for b, nb, T in zip(batches, Bs, Ts)]
        sch = MixerDiffusion(use_timesteps=space_timesteps(self.diffusion_steps, self.sampling_strategy), betas=self.betas).schedule
        if not 0 <= skip < sch.num_timesteps:
            raise ValueError(f"skip_timesteps={skip} outside [0, {sch.num_timesteps})")
        kept, slots, per_row = _history_plan(mode, m.store_influence, keep_history, sch.num_timesteps, skip, self.history_every, m.mixing_mode)
        names = list(kept)
        keys = ("influence_i1", "influence_i2") + (("out1", "out2", "out_influenced") if mode == "eval" else ())
        results = [{"output": None, **{k: [] for k in keys}} for _ in batches]
        if batching == "sequential":
            for i, (b, c, x) in enumerate(zip(batches, conds, xs)):
                bb = dict(b)
                bb["cond"], bb["x_T"] = c, x
                keep = m.store_influence
                if not names:
                    m.store_influence = False
                try:
                    if use_opts:                          # the uniform option path (ddim_sample_loop -> mmdm_begin_opts)
                        out = self._sample(bb, mode, eta=eta, skip_timesteps=skip, seed=seeds[i], step_noise=b.get("step_noise") if form == "noise" else None,
                                           x_start=b.get("x_start"), init_image=b.get("init_image"))
                        results[i] = {"output": out, "influence_i1": m.history_influence_i1, "influence_i2": m.history_influence_i2}
                        if mode == "eval":
                            results[i].update(out1=m.history_out1, out2=m.history_out2, out_influenced=m.history_out_influenced)
                    else:
                        results[i] = self.forward(bb) if mode == "eval" else self.forward_test(bb)
                finally:
                    m.store_influence = keep
            return results
        if batching == "inflight":
            pool = self._pool(max(1, int(inflight)), max(Bs), max(Ts))
            for smp in pool:
                smp.use_schedule(sch)
            # ONE host thread drives every handle (calls dealt round-robin, nothing synchronised in between).  One thread per handle was built
            # and measured (tools/inflight_probe.py: 4 handles 3.65 vs 4.27 ms per item-step) and is not used: graph launches from two host
            # threads crash inside this runtime's hipGraphLaunch (hip::Graph::UpdateStreams) as soon as the threads also capture new shapes,
            # whatever the locking around captures (LAB_NOTES.md, round 5).  Buffers are allocated up front; the calls are C-ABI calls only.
            conds = [c.to(dev, torch.float32).contiguous() for c in conds]
            xs = [x.contiguous() for x in xs]
            need = per_row * sum(nb * T for nb, T in zip(Bs, Ts))
            # the history side outputs of EVERY call are the caller's to keep (as in the sequential and ragged paths): the same budget, summed
            if need > HISTORY_BUDGET_BYTES:
                raise MemoryError(f"history side outputs of {len(Bs)} in-flight calls need {need / 2**30:.1f} GiB; pass fewer batches per call, set "
                                  "model.history_every, or pass keep_history=False")
            cur = torch.cuda.current_stream(dev)
            # calls are queued in windows of a few multiples of `inflight`: output and history buffers are allocated per window (the caching
            # allocator is not touched while a window's calls are being queued), so lazily built inputs of later windows are not needed yet
            win = 4 * len(pool)
            for w0 in range(0, len(conds), win):
                idx = range(w0, min(w0 + win, len(conds)))
                outs = {i: torch.empty_like(xs[i]) for i in idx}
                hists = {i: {nm: torch.empty(slots, 2 * Bs[i], Ts[i], width, device=dev) for nm, width in kept.items()} for i in idx}
                for smp in pool:                     # inputs and buffers were produced on the caller's stream: order every handle's stream behind it
                    smp.stream.wait_stream(cur)
                for i in idx:
                    pool[i % len(pool)].enqueue(conds[i], xs[i], outs[i], hists[i], self.history_every)
                for smp in pool:
                    cur.wait_stream(smp.stream)
                    smp.stream.synchronize()
                for i in idx:
                    results[i]["output"] = outs[i]
                    for k, v in hists[i].items():
                        results[i][k] = list(v.unbind(0))
            return results
        # ragged: motions in call order, cut into groups of <= max_rows frames and <= max_items motions
        groups = pack_groups(Bs, Ts, max_rows, max_items)
        Tm = max(max(Ts), self.num_frames)
        smp = self._sampler_for(_handle_batch(groups, Ts, Tm), Tm)
        smp.use_schedule(sch)
        steps = sch.num_timesteps - skip
        _check_loop_shapes(batches, form, Bs, Ts, steps, "sample_many", 524)

        def budget(frames):
            need = per_row * (frames + 128)
            if need > HISTORY_BUDGET_BYTES:
                raise MemoryError(f"history side outputs of a ragged batch of {frames} frames need {need / 2**30:.1f} GiB; lower max_rows, set "
                                  "model.history_every, or pass keep_history=False")

        options = [_group_options(g, form, seeds, batches, steps, skip) if use_opts else {} for g in groups]
        outs, hists = _run_groups(smp, groups, conds, xs, Ts, options, eta, history=names, history_every=self.history_every, budget=budget)
        for i, nb in enumerate(Bs):
            results[i]["output"] = torch.stack(outs[i], 0)
            if names:
                for k in names:
                    cond_rows = torch.stack([hists[i][j][k][0] for j in range(nb)], 1)      # [slots, b, T, C]
                    unc_rows = torch.stack([hists[i][j][k][1] for j in range(nb)], 1)
                    results[i][k] = list(torch.cat([cond_rows, unc_rows], 1).unbind(0))     # [2b, T, C] per kept step
        return results

    def _sample(self, batch, mode, **loop_kw):
        """loop_kw: ddim_sample_loop's other arguments (eta, skip_timesteps, init_image, x_start, step_noise, seed); none for forward / forward_test."""
        self.mixing.mode = mode
        cond = self.generate_cond(batch)
        B = cond.shape[0]
        T = int(batch["motion_lens"][0])
        self.diffusion_test = MixerDiffusion(use_timesteps=space_timesteps(self.diffusion_steps, self.sampling_strategy), betas=self.betas)
        self.cfg_model = ClassifierFreeSampleModelX2(self.mixing, self.cfg_mixing_weight)
        return self.diffusion_test.ddim_sample_loop(self.cfg_model, (B, T, self.nfeats * 2), noise=batch.get("x_T"), clip_denoised=False,
                                                    progress=True, model_kwargs={"mask": None, "cond": cond}, **{"x_start": None, **loop_kw})

    def forward(self, batch):
        """mixermdm.py:490-548."""
        output = self._sample(batch, "eval")
        m = self.mixing
        return {"output": output, "influence_i1": m.history_influence_i1, "influence_i2": m.history_influence_i2,
                "out1": m.history_out1, "out2": m.history_out2, "out_influenced": m.history_out_influenced}

    def forward_test(self, batch):
        """mixermdm.py:550-602."""
        output = self._sample(batch, "eval_intermediate")
        m = self.mixing
        return {"output": output, "influence_i1": m.history_influence_i1, "influence_i2": m.history_influence_i2}


# ---- stand-alone in2IN, InterGen and MDM samplers; what the many-call drivers share ----------------------------------------------------
def _unwrap_checkpoint(state_dict):
    """A raw state dict, or a Lightning checkpoint {"state_dict": {"model.<key>": ...}} (mixermdm.py:43-59): the ``model.`` prefix is dropped."""
    sd = state_dict["state_dict"] if "state_dict" in state_dict and isinstance(state_dict["state_dict"], dict) else state_dict
    if sd and all(k.startswith("model.") for k in sd):
        sd = {k[len("model."):]: v for k, v in sd.items()}
    return dict(sd)


def _unsupported(fn, *a, **k):
    """Runs a sampler call; a refusal of the library (MMDM_ERR_UNSUPPORTED) becomes NotImplementedError with the library's message."""
    from ._lib import MMDMError
    try:
        return fn(*a, **k)
    except MMDMError as e:
        if e.status == _KeyMask.UNSUPPORTED:
            raise NotImplementedError(str(e)) from None
        raise


def _draw_seed():
    """An un-named seed comes from torch's default generator: torch.manual_seed reproduces a run."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _loop_forms(batches, eta, skip, who, no_opts=None):
    """The rules of a many-call for the loop arguments a batch dict may carry: 'x_start' / 'init_image' for every batch or for none; at eta > 0
    ONE noise form per call -- 'seed' (an un-named one is drawn, in batch order) or 'step_noise'.  no_opts: the refusal of a caller that takes none
    of the options.  -> (any option in use, form "seed" | "noise" | None, seeds per batch)."""
    has = lambda k: [b.get(k) is not None for b in batches]
    for k in ("x_start", "init_image"):
        if any(has(k)) and not all(has(k)):
            raise ValueError(f"{who}: batch {has(k).index(not has(k)[0])} differs from batch 0 in whether it gives {k!r}: give it for every batch or for none")
    use_opts = bool(eta or skip or any(has("x_start")) or any(has("init_image")))
    if use_opts and no_opts:
        raise ValueError(f"{who}: {no_opts}")
    form, seeds = None, [None] * len(batches)
    if eta:
        for i, b in enumerate(batches):
            sd, sn = b.get("seed"), b.get("step_noise")
            if sd is not None and sn is not None:
                raise ValueError(f"{who}: batch {i} gives both 'seed' and 'step_noise'")
            f = "noise" if sn is not None else "seed"
            if form is not None and f != form:
                raise ValueError(f"{who}: batch {i} names its step noise as a {f!r}, batch 0 as a {form!r}: one noise form per call")
            form = f
            if f == "seed":
                seeds[i] = int(sd) if sd is not None else _draw_seed()
    return use_opts, form, seeds


def _check_loop_shapes(batches, form, Bs, Ts, steps, who, width):
    """The shapes of a many-call's 'step_noise' (form "noise"), 'x_start' and 'init_image' entries against their batch's (b, T)."""
    if form == "noise":
        for i, b in enumerate(batches):
            sn = b["step_noise"]
            if sn.dim() != 4 or sn.shape[0] < steps or tuple(sn.shape[1:]) != (Bs[i], Ts[i], width):
                raise ValueError(f"{who}: batch {i}: step_noise [>= {steps}, {Bs[i]}, {Ts[i]}, {width}] expected, got {tuple(sn.shape)}")
    for k in ("x_start", "init_image"):
        for i, b in enumerate(batches):
            if b.get(k) is not None and (b[k].dim() != 3 or b[k].shape[0] != Bs[i]):
                raise ValueError(f"{who}: batch {i}: {k} [{Bs[i]}, T, {width}] expected, got {tuple(b[k].shape)}")


def _group_options(g, form, seeds, batches, steps, skip):
    """sample_ragged_async's keywords for the group g of a many-call with options: motion j of batch i draws (seed_i, noise row j), or takes its slice
    of the batch's buffers."""
    kw = {"skip_timesteps": skip}
    if form == "seed":
        kw["seeds"], kw["noise_rows"] = [seeds[i] for i, _ in g], [j for _, j in g]
    elif form == "noise":
        kw["noise"] = [batches[i]["step_noise"][:steps, j] for i, j in g]
    for k in ("x_start", "init_image"):
        if batches[g[0][0]].get(k) is not None:
            kw[k] = [batches[i][k][j] for i, j in g]
    return kw


def _loop_call(s, cond, x_T, eta=0.0, seed=None, step_noise=None, x_start=None, init_image=None, skip_timesteps=0, start_step=None):
    """One sampling call with the loop's other arguments on a sampler that takes them (single_only 0 / 4).  eta > 0 needs its step noise: step_noise
    [>= S - skip, B, T, 524] or seed (the device generator; with neither, a seed is drawn from torch's default generator).  eta belongs to the call."""
    eta = float(eta)
    if eta < 0:
        raise ValueError(f"eta={eta} must be >= 0")
    if step_noise is not None and seed is not None:
        raise ValueError("give the step noise as a buffer (step_noise=) or as a seed (seed=), not both")
    if eta == 0.0:
        step_noise = seed = None
    elif step_noise is None and seed is None:
        seed = _draw_seed()
    S, skip = s.schedule.num_timesteps, int(skip_timesteps)
    if not 0 <= skip < S:
        raise ValueError(f"skip_timesteps={skip} outside [0, {S})")
    try:
        kw = dict(eta=eta, noise=step_noise[:S - skip] if step_noise is not None else None, seed=seed, x_start=x_start, init_image=init_image, skip_timesteps=skip)
        if start_step is not None:
            return s.sample_from(cond, x_T, start_step, **kw)
        return s.sample(cond, x_T, **kw)
    finally:
        if eta:
            s.set_eta(0.0)


def _refusable_loop_call(s, cond, x_T, loop_kw):
    """The same call on a sampler that refuses the loop's arguments (single_only 1 / 2 / 3): whatever is given is handed to the library, whose refusal
    comes back as NotImplementedError with its message."""
    kw = {k: v for k, v in loop_kw.items() if v is not None and not (k in ("eta", "skip_timesteps") and not v)}
    if "step_noise" in kw:
        kw["noise"] = kw.pop("step_noise")
    if kw.get("eta") and "noise" not in kw and "seed" not in kw:
        kw["seed"] = 0
    if "start_step" in kw:
        return _unsupported(s.sample_from, cond, x_T, kw.pop("start_step"), **kw)
    return _unsupported(s.sample, cond, x_T, **kw)


def pack_groups(Bs, Ts, max_rows=4800, max_items=64):
    """The packing rule of sample_many / invert_many: the motions (batch i, row j) in batch order, cut into ragged groups of <= max_rows frames and
    <= max_items motions (a motion longer than max_rows is a group of its own).  -> list of groups, each a list of (i, j)."""
    groups, cur, rows = [], [], 0
    for i, nb in enumerate(Bs):
        for j in range(nb):
            if cur and (rows + Ts[i] > max_rows or len(cur) >= max_items):
                groups.append(cur)
                cur, rows = [], 0
            cur.append((i, j))
            rows += Ts[i]
    if cur:
        groups.append(cur)
    return groups


def _handle_batch(groups, Ts, Tm):
    """max_batch of the handle of max_frames = Tm that takes every group: its motions, and its frames as rows of the workspace."""
    return max(max(len(g) for g in groups), -(-max(sum(Ts[i] for i, _ in g) for g in groups) // Tm))


def _run_groups(smp, groups, conds, xs, Ts, options, eta=0.0, history=None, history_every=1, budget=None):
    """The ragged launch loop of a many-call: every group queued on the sampler's stream with its keywords (options[k]), eta the call's (the handle is left
    at eta = 0, as a single call leaves it), then the items handed back to their (batch, row).  conds / xs: per batch [b, .] and [b, T, C].  history: the
    names to keep (a list, possibly empty: the two-chain sampler) or None (the one-chain samplers keep none); budget(frames) may refuse a group.
    -> (outs[i][j] = [T_i, C], hists[i][j] = {name: (cond rows, uncond rows), each [slots, T_i, C]} or None): the caller's stream is behind the sampler's."""
    outs = [[None] * len(x) for x in xs]
    hists = [[None] * len(x) for x in xs]
    hkw = {} if history is None else dict(history=history or None, history_every=history_every)
    pend = []
    if eta:
        smp.set_eta(eta)
    try:
        for g, kw in zip(groups, options):
            lens = [Ts[i] for i, _ in g]
            if budget is not None:
                budget(sum(lens))
            items, hist, ev = smp.sample_ragged_async(torch.cat([conds[i][j:j + 1] for i, j in g], 0), [xs[i][j] for i, j in g], lens, **hkw, **kw)
            pend.append((g, items, hist, ev, smp.item_slices() if hist else None))
    finally:
        if eta:
            smp.set_eta(0.0)
    for g, items, hist, ev, slices in pend:
        ev.synchronize()
        for k, (i, j) in enumerate(g):
            outs[i][j] = items[k]
            if hist:                                      # the reference's [2B, T, C] history rows of this motion: its cond row and its uncond row
                o, t = slices[k]
                hists[i][j] = {n: (v[:, 0, o:o + t], v[:, 1, o:o + t]) for n, v in hist.items()}
    torch.cuda.current_stream(smp.device).wait_stream(smp.stream)
    return outs, hists


def _invert_inputs(model, batch):
    """(cond, x_0, B, T) of an inversion call: the model's cond entries and batch["motions"] [B, T, WIDTH]."""
    if batch.get("motions") is None:
        raise ValueError(f"{type(model).__name__}.invert: the batch gives no 'motions' [B, T, {model.WIDTH}]")
    m = batch["motions"]
    if m.dim() != 3:
        raise ValueError(f"{type(model).__name__}.invert: motions [B, T, {model.WIDTH}] expected, got {tuple(m.shape)}")
    return model._inputs(dict(batch, x_T=m, motion_lens=[m.shape[1]]))


def _invert(model, batch, steps):
    from .sampler import invert_steps
    cond, x_0, B, T = _invert_inputs(model, batch)
    s = model._get_sampler(B, T)
    k = invert_steps(steps, s.schedule.num_timesteps)
    return {"latent": _unsupported(s.invert, cond, x_0, k), "steps": k}


def _invert_many(model, batches, batching, steps, max_rows, max_items):
    from .sampler import invert_steps
    who = f"{type(model).__name__}.invert_many"
    if batching not in ("sequential", "ragged"):
        raise ValueError(f'{who}: batching {batching!r} not recognized ("ragged" or "sequential")')
    if batching == "sequential":
        return [_invert(model, b, steps) for b in batches]
    ins = [_invert_inputs(model, b) for b in batches]
    Bs, Ts = [v[2] for v in ins], [v[3] for v in ins]
    groups = pack_groups(Bs, Ts, max_rows, max_items)
    Tm = max(max(Ts), model.num_frames)
    smp = model._get_sampler(_handle_batch(groups, Ts, Tm), Tm)
    k = invert_steps(steps, smp.schedule.num_timesteps)
    outs = [[None] * nb for nb in Bs]
    for g in groups:
        items = _unsupported(smp.invert_ragged, torch.cat([ins[i][0][j:j + 1] for i, j in g], 0), [ins[i][1][j] for i, j in g], [Ts[i] for i, _ in g], k)
        for (i, j), it in zip(g, items):
            outs[i][j] = it
    return [{"latent": torch.stack(o, 0), "steps": k} for o in outs]


class _StandaloneDiffusion(nn.Module):
    """What in2INDiffusion, InterDiffusion and MDM share: parameters under the reference's names, one Sampler handle, the schedule, ragged batching of many calls."""
    WIDTH = 524
    _who = None               # the model's name in the "MI355X only" refusal, when it is not the class name
    _loop_options = True      # False: the handle refuses the loop's options (eta, skip_timesteps, x_start, init_image) by name

    def _apply(self, fn, recurse=True):
        self._dirty = True
        return super()._apply(fn, recurse)

    @property
    def device(self):
        return next(self.parameters()).device

    def load_state_dict(self, state_dict, strict=True):
        sd = {k: v for k, v in state_dict.items() if not k.endswith("sequence_pos_encoder.pe")}
        self._dirty = True
        return super().load_state_dict(sd, strict=strict)

    def _handle_kind(self, legacy):
        """The Sampler keywords that tell the model's handle variants apart (none by default)."""
        return {}

    def _on_schedule(self, s):
        """Runs after the handle took a new schedule."""

    def _get_sampler(self, B, T, legacy=False):
        """The one handle of the model, loaded and on the model's schedule.  A handle is re-built when the variant (_handle_kind(legacy), precision) or the
        device changes or it is too small; growth keeps the previous max_batch of the same variant."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"{self._who or type(self).__name__} runs on an MI355X only: call .to('cuda:N') first (no CPU path)")
        kind = (self._handle_kind(legacy), self.precision)
        s = self._sampler
        same = s is not None and s._kind == kind
        if not same or B > s.cfg.max_batch or T > s.cfg.max_frames or s.device != dev:
            grow = s.cfg.max_batch if same else 1
            if s is not None:
                s.close()
            s = self._make_sampler(max(B, grow), max(T, self.num_frames), dev, **kind[0])
            s._kind = kind
            self._sampler, self._dirty = s, True
        if self._dirty:
            s.load_state_dict(self._sampler_state())
            s.prepare()
            s._strategy = None
            self._dirty = False
        if s._strategy != self.sampling_strategy:
            s.set_schedule(self.sampling_strategy, self.beta_scheduler, self.diffusion_steps)
            self._on_schedule(s)
            s._strategy = self.sampling_strategy
        return s

    def _inputs(self, batch):
        cond = batch["cond"]
        B, T = cond.shape[0], int(batch["motion_lens"][0])
        x_T = batch["x_T"] if batch.get("x_T") is not None else torch.randn(B, T, self.WIDTH, device=self.device)
        if tuple(x_T.shape) != (B, T, self.WIDTH):
            raise ValueError(f"{type(self).__name__}: x_T [{B}, {T}, {self.WIDTH}] expected, got {tuple(x_T.shape)}")
        return cond, x_T, B, T

    def _sample_many(self, batches, batching, max_rows, max_items, eta=0.0, skip_timesteps=0):
        who = f"{type(self).__name__}.sample_many"
        if batching not in ("sequential", "ragged"):
            raise ValueError(f'{who}: batching {batching!r} not recognized ("ragged" or "sequential")')
        eta, skip = float(eta), int(skip_timesteps)
        if eta < 0:
            raise ValueError(f"eta={eta} must be >= 0")
        use_opts, form, seeds = _loop_forms(batches, eta, skip, who)
        if use_opts and not self._loop_options:
            # the library decides: its refusal (mode 1 keeps the option refusals) comes back as NotImplementedError with its message
            cond, x_T, B, T = self._inputs(batches[0])
            _unsupported(self._get_sampler(B, T).sample, cond, x_T, eta=eta, skip_timesteps=skip, seed=seeds[0], x_start=batches[0].get("x_start"),
                         init_image=batches[0].get("init_image"))
            raise NotImplementedError(f"{who}: the loop options are not covered by this sampler")
        if batching == "sequential":
            out = []
            for i, b in enumerate(batches):
                kw = dict(eta=eta, skip_timesteps=skip, seed=seeds[i], step_noise=b.get("step_noise") if form == "noise" else None,
                          x_start=b.get("x_start"), init_image=b.get("init_image")) if use_opts else {}
                out.append({"output": self.forward(b, **kw)["output"]})
            return out
        ins = [self._inputs(b) for b in batches]
        Bs, Ts = [v[2] for v in ins], [v[3] for v in ins]
        groups = pack_groups(Bs, Ts, max_rows, max_items)
        Tm = max(max(Ts), self.num_frames)
        smp = self._get_sampler(_handle_batch(groups, Ts, Tm), Tm)
        S = smp.schedule.num_timesteps
        if not 0 <= skip < S:
            raise ValueError(f"skip_timesteps={skip} outside [0, {S})")
        _check_loop_shapes(batches, form, Bs, Ts, S - skip, who, self.WIDTH)
        options = [_group_options(g, form, seeds, batches, S - skip, skip) if use_opts else {} for g in groups]
        outs, _ = _run_groups(smp, groups, [v[0] for v in ins], [v[1] for v in ins], Ts, options, eta)
        return [{"output": torch.stack(o, 0)} for o in outs]

    def invert(self, batch, steps=None):
        """DDIM inversion of batch["motions"] [B, T, WIDTH] (normalised space) under batch["cond"] -> {"latent": [B, T, WIDTH], "steps": k}: the chain at
        respaced step k (None = all S steps: the x_T of a plain forward).  For k < S, forward(dict(batch, x_T=latent), start_step=k) walks the same levels
        down again."""
        return _invert(self, batch, steps)

    def invert_many(self, batches, batching="ragged", steps=None, max_rows=4800, max_items=64):
        """invert for many batches with sample_many's packing: every latent bit-identical to that batch's own invert call."""
        return _invert_many(self, batches, batching, steps, max_rows, max_items)


class _TextStage:
    """sample_many / invert / invert_many of the text facades (in2IN, InterGen, MDM): the stand-alone sampler's (``_sampler_model``: the facade's
    ``decoder``; MDM is its own) after the text stage.  The one hook: ``_with_cond(batch)`` fills the sampler's cond entries into the batch (a copy; called
    under no_grad).  A class that names an existing method as the hook (``_with_cond = text_process``) binds it as the class is created: a subclass that
    overrides that method names it again."""
    _sampler_model = property(lambda self: self.decoder)

    def _conds(self, batches):
        with torch.no_grad():
            return [self._with_cond(dict(b)) for b in batches]

    def sample_many(self, batches, mode=None, batching="ragged", inflight=None, max_rows=4800, max_items=64, keep_history=None, *, eta=0.0, skip_timesteps=0):
        """The sampler's sample_many (InterDiffusion.sample_many) after the text stage -> one {"output"} per batch, every motion bit-identical to the
        sequential calls.  mode / inflight / keep_history are accepted for generate_for_evaluation's call and unused (one chain, no history side outputs)."""
        return self._sampler_model._sample_many(self._conds(batches), batching, max_rows, max_items, eta, skip_timesteps)

    def invert(self, batch, steps=None):
        """The sampler's invert after the text stage: batch["motions"] [B, T, WIDTH] under the batch's text / cond entries -> {"latent", "steps"}."""
        return _invert(self._sampler_model, self._conds([batch])[0], steps)

    def invert_many(self, batches, batching="ragged", steps=None, max_rows=4800, max_items=64):
        """The sampler's invert_many after the text stage: every latent bit-identical to that batch's own invert call."""
        return _invert_many(self._sampler_model, self._conds(batches), batching, steps, max_rows, max_items)


class in2INDiffusion(_StandaloneDiffusion):
    """Stand-alone sub-model sampler: in2INDiffusion.forward (src/models/in2in.py:285-356), modes "individual"
    (ClassifierFreeSampleModel, [B,T,262]), "interaction" (ClassifierFreeSampleModelMultiple, [B,T,524]) and "dual"
    (ClassifierFreeSampleDualMDM over net_individual + net_interaction, [B,T,524]); output stays in the model's normalised
    space, as in the reference (callers de-normalise: src/scripts/infer/in2IN.py:101-105).
    Handles, one at a time: "interaction" / "dual" run on ``Sampler(single_only=4, cfg_form=1 / 2)`` -- the samplers of single_only 2 / 3 bit for bit, with
    the loop's other arguments (GaussianDiffusion.ddim_sample_loop, gaussian_diffusion.py:946-1069) and ragged batches -- except a call with an explicit
    ``mask``, which builds the single_only 2 / 3 handle and gets its refusal by name; "individual" stays on single_only=1, whose refusal of the loop's
    arguments comes back as NotImplementedError.  ``.precision`` picks the handle's mode."""

    _who = "in2IN"

    def __init__(self, cfg, mode, sampling_strategy="ddim50"):
        super().__init__()
        if mode not in ("individual", "interaction", "dual"):
            raise ValueError(f"in2IN mode {mode!r} not recognized")
        self.cfg, self.mode = cfg, mode
        self.nfeats = cfg.INPUT_DIM
        self.dims = dict(d_latent=cfg.LATENT_DIM, d_ff=cfg.FF_SIZE, d_layers=cfg.NUM_LAYERS)
        self.num_heads = cfg.NUM_HEADS
        self.cfg_weight = cfg.CFG_WEIGHT if "CFG_WEIGHT" in cfg else 0.0
        self.cfg_weight_interaction = cfg.CFG_WEIGHT_INTERACTION if "CFG_WEIGHT_INTERACTION" in cfg else 0.0
        self.cfg_weight_individual = cfg.CFG_WEIGHT_INDIVIDUAL if "CFG_WEIGHT_INDIVIDUAL" in cfg else 0.0
        if mode == "dual":                          # in2in.py:158-162
            self.cfg_composition_weight_func, self.cfg_composition_weight_value = cfg.W_FUNC, cfg.W_VALUE
        self.diffusion_steps = cfg.DIFFUSION_STEPS
        self.betas = get_named_beta_schedule(cfg.BETA_SCHEDULER, self.diffusion_steps)
        self.sampling_strategy = sampling_strategy
        self.beta_scheduler = cfg.BETA_SCHEDULER
        self.num_frames = 300
        self.precision = "fp32"
        self.WIDTH = self.nfeats * (1 if mode == "individual" else 2)
        self._nets = {"individual": [("net_individual", "denoiser1.")], "interaction": [("net_interaction", "denoiser2.")],
                      "dual": [("net_individual", "denoiser1."), ("net_interaction", "denoiser2.")]}[mode]
        from .synthetic import denoiser_shapes
        for net, _ in self._nets:
            for k, shp in denoiser_shapes(net + ".", self.dims["d_latent"], self.dims["d_ff"], self.dims["d_layers"]).items():
                _holder_tree(self, k, torch.zeros(shp))
        self._sampler, self._dirty = None, True

    def _handle_kind(self, legacy):
        """legacy: the single_only 2 / 3 handle of "interaction" / "dual" (a call with a mask)."""
        return {"individual": dict(single_only=1), "interaction": dict(single_only=2) if legacy else dict(single_only=4, cfg_form=1),
                "dual": dict(single_only=3) if legacy else dict(single_only=4, cfg_form=2)}[self.mode]

    @property
    def _loop_options(self):
        return self.mode != "individual"

    def _make_sampler(self, B, T, dev, **kind):
        return Sampler(d_heads=self.num_heads, cfg_scale=self.cfg_weight, cfg_scale_interaction=self.cfg_weight_interaction,
                       cfg_scale_individual=self.cfg_weight_individual, max_batch=B, max_frames=T, device=dev, precision=self.precision, **kind, **self.dims)

    def _sampler_state(self):
        sd = {}
        for net, pfx in self._nets:
            sd.update({pfx + k[len(net) + 1:]: p.data for k, p in self.named_parameters() if k.startswith(net + ".")})
        return sd

    def _on_schedule(self, s):
        if self.mode == "dual":
            s.set_dual_weights(self.cfg_composition_weight_func, self.cfg_composition_weight_value)

    def _inputs(self, batch):
        if self.mode == "dual":                      # in2in.py:299-305
            cond = torch.cat([batch["cond_interaction"], batch["cond_interaction_individual1"], batch["cond_interaction_individual2"],
                              batch["cond_individual_individual1"], batch["cond_individual_individual2"]], dim=1)
        elif self.mode == "interaction":
            cond = torch.cat([batch["cond_interaction"], batch["cond_interaction_individual1"], batch["cond_interaction_individual2"]], dim=1)
        else:
            cond = torch.cat([batch["cond_individual_individual1"]], dim=1)
        B, T = cond.shape[0], int(batch["motion_lens"][0])
        x_T = batch["x_T"] if batch.get("x_T") is not None else torch.randn(B, T, self.WIDTH, device=self.device)
        if tuple(x_T.shape) != (B, T, self.WIDTH):
            raise ValueError(f"in2INDiffusion: x_T [{B}, {T}, {self.WIDTH}] expected, got {tuple(x_T.shape)}")
        return cond, x_T, B, T

    def forward(self, batch, mask=None, eta=0.0, seed=None, step_noise=None, x_start=None, init_image=None, skip_timesteps=0, start_step=None):
        """mask: None as the reference's forward hard-codes (in2in.py:326, 338, 350; a "mask" entry of the batch is never read), or the
        float [B, T, k] key-padding mask for the loop's model_kwargs -- an explicit argument of this port, mode "individual" only.
        The other keywords are the loop's (InterDiffusion.forward's rules): modes "interaction" and "dual".  start_step (every mode): x_T is the chain
        at that respaced step -- the latent of invert(batch, steps=start_step) -- and the loop runs from there (Sampler.sample)."""
        cond, x_T, B, T = self._inputs(batch)
        loop_kw = dict(eta=eta, seed=seed, step_noise=step_noise, x_start=x_start, init_image=init_image, skip_timesteps=skip_timesteps, start_step=start_step)
        if mask is not None or self.mode == "individual":
            s = self._get_sampler(B, T, legacy=mask is not None)
            with _KeyMask(s, mask):                  # model_kwargs = {"mask": mask, "cond": cond} of the loop
                return {"output": _refusable_loop_call(s, cond, x_T, loop_kw)}
        return {"output": _loop_call(self._get_sampler(B, T), cond, x_T, **loop_kw)}

    def sample_many(self, batches, batching="ragged", max_rows=4800, max_items=64, *, eta=0.0, skip_timesteps=0):
        """InterDiffusion.sample_many for this model: batch dicts as forward takes them, every motion bit-identical to that batch's own forward call.
        Mode "individual" runs ragged without the loop's options (NotImplementedError with the library's message otherwise)."""
        return self._sample_many(batches, batching, max_rows, max_items, eta, skip_timesteps)


class in2IN(_TextStage, nn.Module):
    """in2IN(cfg, mode) facade (src/models/in2in.py:14-135) around the stand-alone sampler.  Text conditioning: when the loaded checkpoint
    carries the CLIP tower and the clipTransEncoder_{individual,interaction} heads (in2in.py:24-69), ``text_process`` runs them on the GPU
    (mixermdm_amd.text); otherwise pass the encoded ``cond_*`` entries in the batch or register ``text_encoder(batch, mode, text_name, out_name)``."""

    def __init__(self, cfg, mode):
        super().__init__()
        self.cfg, self.mode = cfg, mode
        self.decoder = in2INDiffusion(cfg, mode, sampling_strategy=cfg.STRATEGY)
        self.text_encoder = None
        self.text_num_heads = 8               # nhead of the clipTransEncoder layers (hard-coded in the reference: in2in.py:27, 43)
        self._text_sd, self._text = None, None

    def load_state_dict(self, state_dict, strict=True):
        """in2IN checkpoint (raw state dict, in2in.py keys): ``decoder.*`` -> the sampler; tower + text heads -> the GPU text stage."""
        dec = {k[len("decoder."):]: v for k, v in state_dict.items() if k.startswith("decoder.")}
        res = self.decoder.load_state_dict(dec, strict=strict)
        pre = ("token_embedding.", "positional_embedding", "clip_transformer.", "ln_final.", "clipTransEncoder_", "clip_ln_")
        txt = {k: v for k, v in state_dict.items() if k.startswith(pre)}
        if "token_embedding.weight" in txt:
            self._text_sd, self._text = txt, None
        return res

    def _text_stage(self, mode):
        from .text import ClipTextTower, TextHead
        dev = next(self.decoder.parameters()).device
        if self._text is None or self._text["tower"].table.device != dev:
            sd = self._text_sd
            heads = sd["clip_transformer.resblocks.0.attn.in_proj_weight"].shape[1] // 64 if "clip_transformer.resblocks.0.attn.in_proj_weight" in sd else 12
            self._text = {"tower": ClipTextTower(sd, "", heads, dev)}
            for m in ("individual", "interaction"):
                if f"clip_ln_{m}.weight" in sd:
                    self._text[m] = TextHead(sd, f"clipTransEncoder_{m}.", f"clip_ln_{m}", self.text_num_heads, dev)
        if mode not in self._text:
            raise ValueError("Mode not recognized")
        return self._text["tower"], self._text[mode]

    def text_process(self, batch, mode=None, text_name="text", out_name="cond"):
        if out_name in batch:
            return batch
        if self.text_encoder is not None:
            return self.text_encoder(batch, mode, text_name, out_name)
        if self._text_sd is None:
            raise NotImplementedError("text encoding (CLIP tower + clipTransEncoder, in2in.py:109-135) is upstream of the HIP path: "
                                      f"put the encoded '{out_name}' in the batch, load a checkpoint that carries the text modules, or set model.text_encoder")
        from .text import tokenize
        tower, head = self._text_stage(mode)
        tok = torch.as_tensor(batch["tokens_" + text_name]) if "tokens_" + text_name in batch else tokenize(batch[text_name])
        batch[out_name] = head(tower(tok), tok)
        return batch

    def decode_motion(self, batch):
        batch.update(self.decoder(batch))
        return batch

    def forward_test(self, batch):
        batch = self._text_all(batch)
        batch.update(self.decode_motion(batch))
        return batch

    def _text_all(self, batch):
        """forward_test's text stage: the cond_* entries of the mode"""
        if self.mode in ("interaction", "dual"):
            batch = self.text_process(batch, "interaction", out_name="cond_interaction")
            batch = self.text_process(batch, "interaction", "text_individual1", "cond_interaction_individual1")
            batch = self.text_process(batch, "interaction", "text_individual2", "cond_interaction_individual2")
        if self.mode == "dual":
            batch = self.text_process(batch, "individual", "text_individual1", "cond_individual_individual1")
            batch = self.text_process(batch, "individual", "text_individual2", "cond_individual_individual2")
        elif self.mode == "individual":
            batch = self.text_process(batch, "individual", out_name="cond_individual_individual1")
        return batch

    _with_cond = _text_all


class InterDiffusion(_StandaloneDiffusion):
    """InterDiffusion (src/models/intergen.py:96-213): InterDenoiser ``net`` under ClassifierFreeSampleModel(cfg.CFG_WEIGHT) in the single-chain DDIM loop,
    [B, T, 524] in the model's normalised space.  Runs on ``Sampler(single_only=4, model2_kind=1)``; ``.precision`` picks the handle's mode (all four).
    ``forward`` also takes the loop's other arguments (GaussianDiffusion.ddim_sample_loop, gaussian_diffusion.py:946-1069), which the reference's call site
    leaves at their defaults (x_start=None, intergen.py:203-212)."""
    WIDTH = 524

    def __init__(self, cfg, sampling_strategy="ddim50"):
        super().__init__()
        self.cfg = cfg
        self.nfeats = cfg.INPUT_DIM
        self.latent_dim, self.ff_size, self.num_layers, self.num_heads = cfg.LATENT_DIM, cfg.FF_SIZE, cfg.NUM_LAYERS, cfg.NUM_HEADS
        self.cfg_weight = cfg.CFG_WEIGHT
        self.diffusion_steps, self.beta_scheduler = cfg.DIFFUSION_STEPS, cfg.BETA_SCHEDULER
        self.sampling_strategy = sampling_strategy
        self.text_dim = 768
        self.num_frames = 300
        self.precision = "fp32"
        if self.nfeats != 262:
            raise NotImplementedError(f"INPUT_DIM={self.nfeats}: the HIP path is built for 262 pose features per person")
        self.betas = get_named_beta_schedule(self.beta_scheduler, self.diffusion_steps)
        from .synthetic import denoiser_shapes
        for k, shp in denoiser_shapes("net.", self.latent_dim, self.ff_size, self.num_layers).items():
            _holder_tree(self, k, torch.zeros(shp))
        self._sampler, self._dirty = None, True

    def _make_sampler(self, B, T, dev):
        return Sampler(d_latent=self.latent_dim, d_ff=self.ff_size, d_layers=self.num_layers, d_heads=self.num_heads, single_only=4, model2_kind=1,
                       cfg_scale=self.cfg_weight, max_batch=B, max_frames=T, device=dev, precision=self.precision)

    def _sampler_state(self):
        return {"denoiser2." + k[len("net."):]: p.data for k, p in self.named_parameters()}

    def forward(self, batch, *, eta=0.0, seed=None, step_noise=None, x_start=None, init_image=None, skip_timesteps=0, start_step=None):
        """intergen.py:184-213 -> {"output": [B, T, 524]}.  eta > 0 needs its step noise: step_noise [>= S - skip, B, T, 524] or seed (the device generator;
        with neither, a seed is drawn from torch's default generator).  start_step: x_T is the chain at that respaced step (Sampler.sample)."""
        cond, x_T, B, T = self._inputs(batch)
        return {"output": _loop_call(self._get_sampler(B, T), cond, x_T, eta=eta, seed=seed, step_noise=step_noise, x_start=x_start, init_image=init_image,
                                     skip_timesteps=skip_timesteps, start_step=start_step)}

    def sample_many(self, batches, batching="ragged", max_rows=4800, max_items=64, *, eta=0.0, skip_timesteps=0):
        """Many forward calls at once (batch dicts with 'cond' [b, 768], 'motion_lens', optionally 'x_T' [b, T, 524]) -> one {"output"} per batch, every
        motion BIT-IDENTICAL to that batch's own forward call on the same x_T and options.  "sequential" = one call after the other; "ragged" = the motions
        packed into ragged batches of <= max_rows frames / <= max_items motions.  eta / skip_timesteps belong to the call; 'seed' / 'step_noise' /
        'x_start' / 'init_image' in the batch dicts follow MixerMDM.sample_many's rules."""
        return self._sample_many(batches, batching, max_rows, max_items, eta, skip_timesteps)


class InterGen(_TextStage, nn.Module):
    """InterGen(cfg) facade (src/models/intergen.py:20-94) around InterDiffusion.  Checkpoint keys: ``decoder.net.*`` (the denoiser), the aliased CLIP tower
    ``token_embedding.* / positional_embedding / clip_transformer.* / ln_final.*`` and the text head ``clipTransEncoder.* / clip_ln.*``; a Lightning
    checkpoint {"state_dict": {"model.<key>": ...}} is unwrapped.  Text: when the checkpoint carries tower and head, ``text_process`` runs them on the GPU
    (mixermdm_amd.text); otherwise put the encoded 'cond' [B, 768] in the batch or set ``text_encoder(batch, mode, text_name, out_name)``."""
    TEXT_PREFIXES = ("token_embedding.", "positional_embedding", "clip_transformer.", "ln_final.", "clipTransEncoder.", "clip_ln.")

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.latent_dim = cfg.LATENT_DIM
        self.decoder = InterDiffusion(cfg, sampling_strategy=cfg.STRATEGY)
        self.text_encoder = None
        self.text_num_heads = 8               # nhead of the clipTransEncoder layers (intergen.py:41)
        self._text_sd, self._text = None, None

    @property
    def device(self):
        return self.decoder.device

    def load_state_dict(self, state_dict, strict=True):
        sd = _unwrap_checkpoint(state_dict)
        unexpected = [k for k in sd if not k.startswith("decoder.") and not k.startswith(self.TEXT_PREFIXES)]
        if strict and unexpected:
            raise RuntimeError("Error(s) in loading state_dict for InterGen:\n\tUnexpected key(s): %s" % unexpected[:8])
        res = self.decoder.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=strict)
        txt = {k: v for k, v in sd.items() if k.startswith(self.TEXT_PREFIXES)}
        if "token_embedding.weight" in txt and "clip_ln.weight" in txt:
            self._text_sd, self._text = txt, None
        return res

    def text_process(self, batch, mode="interaction", text_name="text", out_name="cond"):
        if out_name in batch:
            return batch
        if mode not in ("individual", "interaction"):
            raise ValueError("Mode not recognized")
        if self.text_encoder is not None:
            return self.text_encoder(batch, mode, text_name, out_name)
        if self._text_sd is None:
            raise NotImplementedError("text encoding (CLIP tower + clipTransEncoder, intergen.py:68-94) is upstream of the HIP path: "
                                      f"put the encoded '{out_name}' in the batch, load a checkpoint that carries the text modules, or set model.text_encoder")
        from .text import ClipTextTower, TextHead, tokenize
        dev = self.device
        if self._text is None or self._text[0].table.device != dev:
            sd = self._text_sd
            heads = sd["clip_transformer.resblocks.0.attn.in_proj_weight"].shape[1] // 64 if "clip_transformer.resblocks.0.attn.in_proj_weight" in sd else 12
            self._text = (ClipTextTower(sd, "", heads, dev), TextHead(sd, "clipTransEncoder.", "clip_ln", self.text_num_heads, dev))
        tower, head = self._text
        tok = torch.as_tensor(batch["tokens_" + text_name]) if "tokens_" + text_name in batch else tokenize(batch[text_name])
        batch[out_name] = head(tower(tok), tok)
        return batch

    _with_cond = text_process

    def decode_motion(self, batch):
        batch.update(self.decoder(batch))
        return batch

    def forward_test(self, batch):
        """intergen.py:63-66: the batch, with 'cond' and 'output' [B, T, 524] (normalised space) added."""
        batch = self.text_process(batch)
        batch.update(self.decode_motion(batch))
        return batch

    def forward(self, batch, **loop_kw):
        """Sampling with the loop's other arguments (InterDiffusion.forward's keywords)."""
        batch = self.text_process(batch)
        batch.update(self.decoder(batch, **loop_kw))
        return batch


class MDM(_TextStage, _StandaloneDiffusion):
    """MDM(cfg, num_frames, sampling_strategy) (src/models/mdm.py:9-66, 195-231): MDMDenoiser ``model`` under ClassifierFreeSampleModel(cfg.CFG_WEIGHT),
    one person, [B, T, 262]; runs on ``Sampler(single_only=1, model1_kind=1)`` -- precision "fp32" or "fp32_split", as the handle allows.  Parameters:
    ``model.*`` and ``embed_text.*``; text goes through MDM's own CLIP model + embed_text (mixermdm_amd.text.MdmTextHead) when the checkpoint carries
    ``clip_model.*``, else pass 'cond' [B, LATENT_DIM] (what embed_text hands the denoiser).  The loop options are refused by the library for this mode:
    NotImplementedError with its message."""
    WIDTH = 262
    _loop_options = False
    _sampler_model = property(lambda self: self)

    def __init__(self, cfg, num_frames=300, sampling_strategy="ddim50"):
        super().__init__()
        self.cfg = cfg
        self.nfeats = cfg.INPUT_DIM
        self.latent_dim, self.ff_size, self.num_layers, self.num_heads = cfg.LATENT_DIM, cfg.FF_SIZE, cfg.NUM_LAYERS, cfg.NUM_HEADS
        self.cfg_weight = cfg.CFG_WEIGHT
        self.diffusion_steps, self.beta_scheduler = cfg.DIFFUSION_STEPS, cfg.BETA_SCHEDULER
        self.sampling_strategy = sampling_strategy
        self.num_frames = num_frames
        self.precision = "fp32"
        self.text_encoder = None
        self.clip_heads = 8                   # CLIP ViT-B/32 text tower: width 512, 8 heads (mdm.py:72)
        if self.nfeats != 262:
            raise NotImplementedError(f"INPUT_DIM={self.nfeats}: the HIP path is built for 262 pose features per person")
        self.betas = get_named_beta_schedule(self.beta_scheduler, self.diffusion_steps)
        from .synthetic import mdm_denoiser_shapes
        for k, shp in mdm_denoiser_shapes("model.", self.latent_dim, self.ff_size, self.num_layers).items():
            _holder_tree(self, k, torch.zeros(shp))
        _holder_tree(self, "embed_text.weight", torch.zeros(self.latent_dim, 512))
        _holder_tree(self, "embed_text.bias", torch.zeros(self.latent_dim))
        self._sampler, self._dirty = None, True
        self._text_sd, self._text = None, None

    def load_state_dict(self, state_dict, strict=True):
        sd = _unwrap_checkpoint(state_dict)
        clip_sd = {k: v for k, v in sd.items() if k.startswith("clip_model.")}
        res = super().load_state_dict({k: v for k, v in sd.items() if not k.startswith("clip_model.")}, strict=strict)
        if "clip_model.token_embedding.weight" in clip_sd:
            self._text_sd, self._text = clip_sd, None
        return res

    def _make_sampler(self, B, T, dev):
        return Sampler(d_latent=self.latent_dim, d_ff=self.ff_size, d_layers=self.num_layers, d_heads=self.num_heads, single_only=1, model1_kind=1,
                       cfg_scale=self.cfg_weight, max_batch=B, max_frames=T, device=dev, precision=self.precision)

    def _sampler_state(self):
        return {"denoiser1." + k[len("model."):]: p.data for k, p in self.named_parameters() if k.startswith("model.")}

    def generate_cond(self, batch):
        """mdm.py:141-149."""
        if "cond" in batch:
            return batch["cond"]
        if self.text_encoder is not None:
            return self.text_encoder(batch)
        if self._text_sd is None:
            raise NotImplementedError("text encoding (MDM's CLIP ViT-B/32 + embed_text, mdm.py:100-121) is upstream of the HIP path: put the encoded 'cond' "
                                      "[B, LATENT_DIM] in the batch, load a checkpoint that carries clip_model.*, or set model.text_encoder")
        from .text import MdmTextHead, tokenize_mdm
        dev = self.device
        if self._text is None or self._text.w.device != dev:
            sd = dict(self._text_sd)
            sd["embed_text.weight"], sd["embed_text.bias"] = self.embed_text.weight.data, self.embed_text.bias.data
            self._text = MdmTextHead(sd, "", self.clip_heads, dev)
        tok = torch.as_tensor(batch["tokens_mdm_text"]) if "tokens_mdm_text" in batch else tokenize_mdm(batch["text"])
        return self._text(tok)

    def forward(self, batch, **loop_kw):
        """mdm.py:195-228 -> {"output": [B, T, 262]}.  loop_kw (eta, seed, step_noise, x_start, init_image, skip_timesteps): handed to the library, whose
        refusal for this mode comes back as NotImplementedError."""
        b = dict(batch)
        b["cond"] = self.generate_cond(batch)
        cond, x_T, B, T = self._inputs(b)
        return {"output": _refusable_loop_call(self._get_sampler(B, T), cond, x_T, loop_kw)}

    def forward_test(self, batch):
        return self.forward(batch)

    def _with_cond(self, batch):
        batch["cond"] = self.generate_cond(batch)
        return batch
