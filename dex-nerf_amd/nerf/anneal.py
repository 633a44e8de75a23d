"""Coarse-to-fine positional encoding (BARF, Lin et al. 2021, eq. 14) around the fused network kernels.

Band k of an encoding with L bands has the amplitude a_k = (1 - cos(pi clamp(p L - k, 0, 1))) / 2 at progress p = clamp((it - start) /
(end - start), 0, 1); the raw x, y, z columns keep amplitude 1.  The encoding lives inside the fused kernels, so the amplitude is applied
where it is the same thing: as a per-column scale of the fp32 weights that multiply the encoding, W (a * enc) = (W diag(a)) enc, before
they are packed (include/dexnerf_hip_anneal.h).  Forward and input gradient of every precision come out of the unchanged kernels; the
weight gradient is that of the scaled weights times the same column scale (EncodingAnneal.scale_grads, which the fused steps call).

The table is formed on the device from the training loop's iteration counter (the RNG record's `nxt` word), so a replayed HIP graph
follows the schedule by itself."""
import ctypes

import torch

from . import _ops
from ._hip import check, f32c, lib, ptr, stream


class EncodingAnneal:
    """The schedule, its device table and the scaled weight copies of the models it is attached to.

    attach(*models)     the models read their packed weights through this schedule from now on (detach(): no longer)
    advance(rng_state)  the table for the iteration `rng_state` is about to run (read on the device; capturable)
    set_iteration(it)   the table for an explicit iteration (renders, evaluation of a mid-schedule checkpoint)
    amplitudes()        the table (L_xyz + L_dir) fp32 on the device: xyz bands, then view-direction bands

    Both advance() and set_iteration() bump `version`, which is part of every attached model's param_key(): the packed streams
    are rebuilt from freshly scaled copies of the CURRENT weights.  Before the first of them the table is the one of iteration 0."""

    def __init__(self, start, end, anneal_dir=True):
        self.start, self.end = float(start), float(end)
        if not (0.0 <= self.start <= self.end < float("inf")):
            raise ValueError(f"EncodingAnneal: start and end are iterations with 0 <= start <= end (got {start!r}, {end!r})")
        self.anneal_dir = bool(anneal_dir)
        self.version = 0
        self.iteration = 0        # the latest set_iteration() (advance() reads the device counter: not tracked here)
        self.l_xyz = self.l_dir = None
        self.amp = None
        self.models = []
        self._copies = {}         # id(model) -> {index in linear_modules(): scaled copy}

    # ---- models -------------------------------------------------------------------------------------------------------
    def attach(self, *models):
        models = [m for m in models if m is not None]
        for m in models:
            l_dir = m.num_encoding_fn_dir if m.use_viewdirs else 0
            if self.l_xyz is None:
                self.l_xyz, self.l_dir = int(m.num_encoding_fn_xyz), int(l_dir)
            if (int(m.num_encoding_fn_xyz), int(l_dir)) != (self.l_xyz, self.l_dir):
                raise ValueError(f"EncodingAnneal.attach: the models must agree on L_xyz / L_dir (have {self.l_xyz} / {self.l_dir}, got "
                                 f"{m.num_encoding_fn_xyz} / {l_dir})")
            if not m.fused_ok():
                raise ValueError("EncodingAnneal.attach: a network outside the fused kernels (W in {128, 256}, L_xyz in {6, 10}, L_dir = 4)")
            other = getattr(m, "_encoding_anneal", None)
            if other is not None and other is not self:
                raise ValueError("EncodingAnneal.attach: the model already has another schedule attached")
        for m in models:
            if getattr(m, "_encoding_anneal", None) is not self:
                m._encoding_anneal = self
                self.models.append(m)
        if self.amp is None and models:
            self.set_iteration(self.iteration, device=next(models[0].parameters()).device)
        return self

    def detach(self):
        for m in self.models:
            m._encoding_anneal = None
        self.models, self._copies = [], {}
        self.version += 1

    # ---- the table ----------------------------------------------------------------------------------------------------
    def _launch_table(self, rng_state, iteration, device):
        if self.l_xyz is None:
            raise RuntimeError("EncodingAnneal: attach() the models first (they decide L_xyz / L_dir)")
        if self.amp is None:
            if device.type != "cuda":
                raise RuntimeError("EncodingAnneal: the schedule runs on the ROCm device (models on the host have no fused kernels)")
            self.amp = torch.zeros(self.l_xyz + self.l_dir, dtype=torch.float32, device=device)
        check(lib().dn_encoding_anneal_amplitudes(ptr(rng_state), int(iteration), self.start, self.end, self.l_xyz, self.l_dir,
                                                  int(self.anneal_dir), ptr(self.amp), stream()), "dn_encoding_anneal_amplitudes")
        self.version += 1

    def advance(self, rng_state):
        """The table of the iteration `rng_state` (device record {seed_lo, seed_hi, cur, nxt}) runs next: its `nxt` word."""
        assert rng_state.dtype == torch.int32 and rng_state.numel() == 4
        self._launch_table(rng_state, 0, rng_state.device)

    def set_iteration(self, it, device=None):
        self.iteration = int(it)
        if device is None:
            device = self.amp.device if self.amp is not None else next(self.models[0].parameters()).device
        self._launch_table(None, self.iteration, device)

    def amplitudes(self):
        return self.amp

    # ---- weights and gradients ----------------------------------------------------------------------------------------------
    @staticmethod
    def affected(model):
        """Indices, in linear_modules() order, of the layers that read an encoding: layer1, the wide trunk layers, layers_dir.0."""
        idx = [0] + [1 + i for i in model.skip_layers]
        if model.use_viewdirs:
            idx.append(model.num_layers)
        return idx

    def _copy_lists(self, model, weights):
        """(fp32 sources, the same list with the affected entries replaced by this object's copy buffers, both pointer arrays)."""
        copies = self._copies.setdefault(id(model), {})
        src = [f32c(w.detach()) for w in weights]
        out = list(src)
        for i in self.affected(model):
            buf = copies.get(i)
            if buf is None or buf.shape != src[i].shape or buf.device != src[i].device:
                buf = copies[i] = torch.empty_like(src[i])
            out[i] = buf
        n = len(src)
        return src, out, (ctypes.c_void_p * n)(*[t.data_ptr() for t in src]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in out])

    def scaled_weights(self, model, weights):
        """`weights` (linear_modules() order) with the entries of the affected layers replaced by copies scaled from the CURRENT
        values (one launch, dn_encoding_anneal_scale_weights).  The copies are this object's: the next call overwrites them."""
        src, out, wp, sp = self._copy_lists(model, weights)
        desc = _ops._desc(model.desc_kwargs())
        check(lib().dn_encoding_anneal_scale_weights(ctypes.byref(desc), wp, ptr(self.amp), sp, stream()), "dn_encoding_anneal_scale_weights")
        self._keep = src      # sources alive until the kernel has run on this stream
        return out

    def scaled_weights_pair(self, model_a, model_b):
        """scaled_weights() of the current weights of two attached models in ONE launch: (list_a, list_b)."""
        lists = [self._copy_lists(m, [lin.weight for lin in m.linear_modules()]) for m in (model_a, model_b)]
        da, db = (_ops._desc(m.desc_kwargs()) for m in (model_a, model_b))
        check(lib().dn_encoding_anneal_scale_weights_pair(ctypes.byref(da), lists[0][2], lists[0][3], ctypes.byref(db), lists[1][2], lists[1][3],
                                                          ptr(self.amp), stream()), "dn_encoding_anneal_scale_weights_pair")
        self._keep = (lists[0][0], lists[1][0])
        return lists[0][1], lists[1][1]

    def scale_grads(self, model, views):
        """dL/dW = (dL/dW_eff) diag(a), in place on `views` = [(dW, db)] in linear_modules() order (dn_encoding_anneal_scale_grads).
        The arrays must hold one backward's contribution only."""
        gp = (ctypes.c_void_p * len(views))(*[w.data_ptr() for w, _ in views])
        desc = _ops._desc(model.desc_kwargs())
        check(lib().dn_encoding_anneal_scale_grads(ctypes.byref(desc), ptr(self.amp), gp, stream()), "dn_encoding_anneal_scale_grads")

    def scale_grads_pair(self, model_a, views_a, model_b, views_b):
        """scale_grads() of two networks in ONE launch."""
        ga = (ctypes.c_void_p * len(views_a))(*[w.data_ptr() for w, _ in views_a])
        gb = (ctypes.c_void_p * len(views_b))(*[w.data_ptr() for w, _ in views_b])
        da, db = (_ops._desc(m.desc_kwargs()) for m in (model_a, model_b))
        check(lib().dn_encoding_anneal_scale_grads_pair(ctypes.byref(da), ga, ctypes.byref(db), gb, ptr(self.amp), stream()),
              "dn_encoding_anneal_scale_grads_pair")

    # ---- checkpoints ------------------------------------------------------------------------------------------------------------
    def state_dict(self, iteration=None):
        """start, end, the anneal_dir flag and the iteration (given: the number of training steps taken, which a resumed loop passes as
        first_iteration; else the latest set_iteration())."""
        return dict(start=self.start, end=self.end, anneal_dir=self.anneal_dir, iteration=int(self.iteration if iteration is None else iteration))

    @classmethod
    def from_state_dict(cls, state):
        anneal = cls(state["start"], state["end"], state["anneal_dir"])
        anneal.iteration = int(state["iteration"])
        return anneal
