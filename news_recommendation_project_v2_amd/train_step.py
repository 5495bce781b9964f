"""One training step of config 5 on the MI355X.

Replaces the body of ``AttentionAttentionTrainer.train_one_epoch``
(trainer.py:1030-1071) for one batch:

  first_res  = token_model(tok, mask)                  # = g_mlp_LN(last valid token)
  second_res = first_res[hist] * hist_mask             # padded [B, h_max, D]
  outputs    = final_attention(second_res, hist_mask)  # train mode: dropout p = 0.1
  res        = cosine(outputs.repeat(2, 1), first_res[pos ‖ neg])
  loss       = MarginRankingLoss(2)(res[:B], res[B:], 1)
  loss.backward(); clip_grad_norm_(0.5); AdamW(lr 1e-6).step()

as ONE library call per batch (``nr_final_train_step``, csrc/final_train.hip;
no autograd, no torch kernels inside the step):
  * the token model is the g_mlp LayerNorm of the U unique news' last rows;
  * FinalAttention runs once per VALID history slot (Hs = sum h_i rows packed in
    CSR order, zero-padded to a multiple of 64): the reference's padded slots
    are masked to zero weight, so they carry no gradient and skipping them is
    exact; dropout is fused into the ReLU GEMM epilogues with a counter-hash
    stream, its backward into the data-grad GEMMs (the mask is recovered from
    the saved outputs);
  * bf16: the data-grad GEMMs also write the bias gradients (f32 column sums)
    from their epilogues, and the weight-grad GEMMs read the row-major
    activations through transposed LDS reads (no transposed copies);
  * pooling forward / backward, cosine + margin loss, scatter-add of the
    history gradient and the LayerNorm-parameter reductions are HIP kernels;
    the global grad norm and AdamW (clip coefficient folded in) are two more
    launches in ``optimizer_step``.

Parameters live in ONE flat f32 buffer (master weights; the torch modules'
parameters are re-pointed at views of it, so ``state_dict()`` is always
current), with a flat bf16 mirror for the bf16 compute dtype.  Only the
parameters that receive gradients are in it — exactly the set torch's AdamW
updates (the token model's attention / g_mlp weights and attn_layernorm get no
gradient because MyLayer discards them, attention.py:193).
"""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import NewsRecHIPError
from .ops import _pad64

D = 1024
H = 4096
DROP_P = 0.1
MARGIN = 2.0  # MarginRankingLoss(2), trainer.py:985
_BLK = "latent.cross_attend_blocks."  # LatentAttentionModel's parameter names in the flat buffer


@dataclass
class TrainBatch:
    """Device-side batch: the output of ``attention_attention_train_collate_fn``
    in CSR form (data_utils.py:893-915).

    tok_last  [U, D] f32/f16  each unique news' last valid token state
    hist_idx  [Hs] int32      history slots, indices into the U rows
    hist_off  [B+1] int64     CSR offsets of the B batch rows
    pos, neg  [B] int32       positive / negative news, indices into the U rows
    """
    tok_last: torch.Tensor
    hist_idx: torch.Tensor
    hist_off: torch.Tensor
    pos: torch.Tensor
    neg: torch.Tensor

    @property
    def B(self) -> int:
        return self.pos.numel()


@dataclass
class ContrastiveBatch:
    """A ``TrainBatch`` (its ``pos`` / ``neg`` are not read; ``None`` is fine) plus the
    InfoNCE loss's inputs (data_utils.contrastive_batch_csr):

    cand    [Cn] int32        candidate columns, indices into the U rows, -1 = pad
    target  [B] int32         the column of each row's positive
    mask    [B, Cn] uint8     1 = the column is left out for that row; None = no mask
    """
    batch: TrainBatch
    cand: torch.Tensor
    target: torch.Tensor
    mask: Optional[torch.Tensor] = None


def _check_loss_out(t: torch.Tensor, dev) -> torch.Tensor:
    d = torch.device(dev)
    if (t.dtype != torch.float32 or t.numel() < 1 or not t.is_contiguous() or t.device.type != d.type
            or (d.index is not None and t.device.index != d.index)):
        raise NewsRecHIPError("loss_out must be a contiguous float32 tensor with >= 1 element on the step's device")
    return t


class _FlatTrainStep:
    """What the two config-5 steps share: the token LayerNorm's and the pooler's
    parameters adopted into one flat f32 buffer (with gradient, AdamW state and,
    for the bf16 compute dtype, a bf16 mirror), the native step as ONE library
    call per batch, and clip + AdamW as one more.  A subclass describes its native
    step in the attributes below and sets the struct fields only it has (``_fill_args``)."""

    _what = "train step"  # names the step in the dtype error
    _prefix = ""          # of the pooler's parameter names in ``names``
    _args: type           # the native step's args struct (_lib.*TrainArgs)
    _step_fn: str         # library entry points: the step and its workspace size
    _workspace_fn: str
    _contrastive_fn: Optional[str] = None  # the step with the InfoNCE loss (ContrastiveBatch), when it has one
    _pmap: dict           # struct field -> parameter name (``g_`` + field is its gradient)
    _mirrored: tuple      # the fields read in the compute dtype (``cviews``), the GEMM weights

    def __init__(self, token_model, pooler, dtype, lr, betas, eps, weight_decay, max_norm, seed, device,
                 temperature: float = 1.0):
        if dtype not in (torch.float32, torch.bfloat16):
            raise NewsRecHIPError(f"{self._what} dtype must be float32 or bfloat16")
        if not temperature > 0:
            raise NewsRecHIPError("temperature must be positive")
        self.temperature = float(temperature)  # tau of the InfoNCE loss (ContrastiveBatch steps)
        layers = list(token_model.encoder.layer)
        if len(layers) != 1:
            raise NewsRecHIPError("training supports NUM_HIDDEN_LAYERS == 1 (config.py:35)")
        self.device = dev = device or torch.device("cuda")
        self.dtype = dtype
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.seed, self.step_count = seed, 0
        self.ln = layers[0].g_mlp_layernorm
        self.ln_eps = float(self.ln.eps)
        self.pooler = pooler
        named = {"ln.weight": self.ln.weight, "ln.bias": self.ln.bias,
                 **{self._prefix + n: p for n, p in pooler.named_parameters()}}
        self.names, self._mod_params = list(named), list(named.values())  # the modules' own Parameters
        # every slice starts at a multiple of 64 floats, so every view is a valid GEMM operand
        offs = list(itertools.accumulate(((p.numel() + 63) // 64 * 64 for p in self._mod_params), initial=0))
        self.n_flat = offs[-1]
        self.flat = torch.zeros(self.n_flat, dtype=torch.float32, device=dev)
        self.grad, self.m, self.v = (torch.zeros_like(self.flat) for _ in range(3))
        self.flat16 = torch.zeros_like(self.flat, dtype=torch.bfloat16) if dtype == torch.bfloat16 else None
        views = lambda buf: {n: buf[o:o + p.numel()].view(p.shape) for (n, p), o in zip(named.items(), offs)}
        self.views, self.gviews = views(self.flat), views(self.grad)
        self.cviews = views(self.flat16) if self.flat16 is not None else dict(self.views)
        with torch.no_grad():
            for prm, v in zip(self._mod_params, self.views.values()):
                v.copy_(prm.detach().to(dev, torch.float32))
                prm.data = v  # the module now reads the master weights
            if self.flat16 is not None:
                self.flat16.copy_(self.flat)
        self._mirror_version = self._weights_version()
        self.sumsq, self.loss = (torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(2))
        self._ws = None  # the native step's workspace
        self._users = None

    def _fill_args(self, a) -> None:
        """Set the struct fields only this step has."""

    def _weights_version(self) -> tuple:
        """Version counters of everything that can write the master weights outside
        AdamW: the flat buffer and its ``views``, and the modules' Parameters -- one
        keeps its own counter through ``.data =``, so load_state_dict on a wrapped module
        moves only the Parameter's.  AdamW (a call through raw pointers) moves neither."""
        return (self.flat._version,) + tuple(p._version for p in self._mod_params)

    def _refresh_mirror(self) -> None:
        """Rewrite the bf16 weight mirror when the master weights changed outside
        AdamW (load_state_dict on the wrapped modules, an edit through ``views``)."""
        v = self._weights_version()
        if self.flat16 is not None and v != self._mirror_version:
            with torch.no_grad():
                self.flat16.copy_(self.flat)
        self._mirror_version = v

    def forward_backward(self, batch: "TrainBatch | ContrastiveBatch", loss_out: torch.Tensor | None = None):
        """Loss (device scalar, written to ``loss_out`` when given) and gradients
        into ``self.grad`` as ONE library call: the forward, the loss -- the margin
        loss of a ``TrainBatch``, InfoNCE at ``self.temperature`` over the candidate
        columns of a ``ContrastiveBatch`` -- and the whole backward of the batch.  The
        step rewrites every gradient slice, so there is no ``grad.zero_()`` (the
        alignment gaps stay zero from construction).
        Returns (loss, users, None): users = the pooled users [B, D] f32.  Both are
        views of buffers the next call overwrites in place (on the stream); clone
        them to keep a step's values."""
        spec = None
        if isinstance(batch, ContrastiveBatch):
            if self._contrastive_fn is None:
                raise NewsRecHIPError(f"the {self._what} has no contrastive entry")
            cb, batch = batch, batch.batch
            B = batch.hist_off.numel() - 1
            spec = _lib.ContrastiveSpec()
            spec.Cn = ops._check_contrastive(cb.cand, cb.target, cb.mask, B)
            ops._dev(cb.cand, cb.target, cb.mask, batch.tok_last)
            spec.cand, spec.target = cb.cand.data_ptr(), cb.target.data_ptr()
            spec.mask = cb.mask.data_ptr() if cb.mask is not None else None
            spec.inv_tau = 1.0 / self.temperature
        else:
            B = batch.B
        U, Hs = batch.tok_last.shape[0], batch.hist_idx.numel()
        lib = _lib.load()
        self._refresh_mirror()
        dt = ops.TOKEN_DT[self.dtype]
        with torch.cuda.device(self.device):  # the native layout depends on the current device's CU count
            if spec is None:
                need = int(getattr(lib, self._workspace_fn)(dt, B, U, Hs))
            else:
                need = int(getattr(lib, self._contrastive_fn + "_workspace_bytes")(dt, B, U, Hs, spec.Cn))
        self._ws = ops.grow_workspace(self._ws, need, self.device)
        if self._users is None or self._users.shape[0] < B:
            self._users = torch.empty((B, D), dtype=torch.float32, device=self.device)
        tok = batch.tok_last.contiguous()
        hi, ho = batch.hist_idx.to(torch.int32).contiguous(), batch.hist_off.to(torch.int64).contiguous()
        if spec is None:
            pos, neg = batch.pos.to(torch.int32).contiguous(), batch.neg.to(torch.int32).contiguous()
        else:
            pos = neg = None  # (not read by the contrastive entry)
        a = self._args()
        a.dtype, a.tok_dtype, a.B, a.U, a.Hs, a.margin = dt, ops.TOKEN_DT[tok.dtype], B, U, Hs, MARGIN
        self._fill_args(a)
        a.tok_last, a.hist_idx, a.hist_off = (t.data_ptr() for t in (tok, hi, ho))
        a.pos, a.neg = (t.data_ptr() if t is not None else None for t in (pos, neg))
        for f, name in self._pmap.items():
            src = self.cviews if f in self._mirrored else self.views
            setattr(a, f, src[name].data_ptr())
            setattr(a, "g_" + f, self.gviews[name].data_ptr())
        loss = self.loss if loss_out is None else _check_loss_out(loss_out, self.device)
        a.loss, a.users, a.sumsq = loss.data_ptr(), self._users.data_ptr(), self.sumsq.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if spec is None:
            _lib.check(getattr(lib, self._step_fn)(ctypes.byref(a), self._ws.data_ptr(), self._ws.numel(), stream),
                       self._step_fn)
        else:
            _lib.check(getattr(lib, self._contrastive_fn)(ctypes.byref(a), ctypes.byref(spec), self._ws.data_ptr(),
                                                          self._ws.numel(), stream), self._contrastive_fn)
        # alive until the stream has run the step
        self._keep = (tok, hi, ho, pos, neg, cb if spec is not None else None)
        return loss, self._users[:B], None

    def optimizer_step(self) -> None:
        """clip_grad_norm_(max_norm) + AdamW in one launch (trainer.py:1067-1069): the
        squared grad norm was summed by the step itself (``sumsq``), and the same
        launch rewrites the bf16 weight mirror."""
        self.step_count += 1
        ops.adamw(self.flat, self.grad, self.m, self.v, self.step_count, self.lr, self.betas, self.eps, self.wd,
                  self.max_norm, self.sumsq if self.max_norm > 0 else None, self.flat16)
        if hasattr(self.pooler, "_hip_cache"):
            self.pooler._hip_cache = {}  # keyed on data_ptr() and _version, which AdamW moved neither of

    def step(self, batch: "TrainBatch | ContrastiveBatch") -> torch.Tensor:
        """One full step; returns this step's loss as its own device scalar (a
        fresh allocation the step writes, so no copy launch)."""
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        self.forward_backward(batch, loss_out=out)
        self.optimizer_step()
        return out

    def grad_dict(self) -> dict:
        return dict(self.gviews)


class FinalAttentionTrainStep(_FlatTrainStep):
    """The module docstring's step: ``FinalAttention`` pools (``nr_final_train_step``, csrc/final_train.hip)."""

    _args, _step_fn, _workspace_fn = _lib.FinalTrainArgs, "nr_final_train_step", "nr_final_train_workspace_bytes"
    _contrastive_fn = "nr_final_train_step_contrastive"
    _pmap = {"tok_g": "ln.weight", "tok_b": "ln.bias", "W5": "linear5.weight",
             **{f"W{i}": f"linear{i}.weight" for i in range(1, 5)},
             **{f"b{i}": f"linear{i}.bias" for i in range(1, 5)}}
    _mirrored = ("W1", "W2", "W3", "W4", "W5")

    def __init__(self, token_model, final_attention, dtype: torch.dtype = torch.bfloat16, lr: float = 1e-6,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, max_norm: float = 0.5,
                 dropout: float = DROP_P, seed: int = 1234, device=None, temperature: float = 1.0):
        super().__init__(token_model, final_attention, dtype, lr, betas, eps, weight_decay, max_norm, seed, device,
                         temperature)
        # CUs the persistent GEMMs spread one 256x256 tile round over (multiple of the 8 XCDs)
        self._ncu = torch.cuda.get_device_properties(self.device).multi_processor_count // 8 * 8
        self.p = dropout
        self._scratch = {}  # _buf's named buffers

    def _fill_args(self, a) -> None:
        a.p = self.p
        a.seed[:] = [self.layer_seed(layer) for layer in (1, 2, 3)]

    # ------------------------------------------------------------------ helpers
    def _buf(self, name: str, shape, dtype) -> torch.Tensor:
        t = self._scratch.get(name)
        n = int(np.prod(shape))
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(max(n, 1), dtype=dtype, device=self.device)
            self._scratch[name] = t
        return t[:n].view(shape)

    # _tail_rows / _relu_gemm: the Python driver of the split-K tail the native
    # step runs (final_train.hip main_rows / relu_gemm), kept as its test double
    # (tests/test_train.py test_gpu_split_k_tail_matches_full_gemm).
    def _tail_rows(self, M: int, N: int, K: int) -> int:
        """Rows of a bf16 GEMM that fill whole rounds of 256x256 tiles over the CUs
        (the rest, a few tiles that would hold one CU each for a full tile time,
        run as K-slices instead); M when no such split pays -- and at K <= 1024,
        where the persistent kernel's half-tile tail is the cheaper form
        (final_train.hip split_tail)."""
        if self.dtype != torch.bfloat16 or N % 256 or K % 512 or K <= 1024 or M % 256 == 0:
            return M
        ncu = self._ncu
        ntn = N // 256
        if ncu % ntn:
            return M
        m_main = M // (256 * (ncu // ntn)) * (256 * (ncu // ntn))
        tail_tiles = -(-(M - m_main) // 256) * ntn
        return m_main if m_main > 0 and tail_tiles * 4 <= ncu else M

    def _relu_gemm(self, a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, seed: int = 0,
                   y: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
        """gemm_relu_dropout (y None) or gemm_drelu (y = forward output).  When the
        last round of 256x256 tiles would be a few tiles (M just past a multiple
        of 16 M-tiles at N = 4096: M = 8,320 -> 512 + 16 tiles, the 16 costing a
        whole tile time), those rows run as 8 K-slices in one grouped launch plus
        nr_splitk_fixup (sum + bias + the same epilogue / dropout mask)."""
        M, K = a.shape
        N = w.shape[0]
        mm = self._tail_rows(M, N, K)
        if mm > 0:
            if y is None:
                ops.gemm_relu_dropout(a[:mm], w, bias, seed, self.p, out=out[:mm])
            else:
                ops.gemm_drelu(a[:mm], w, y[:mm], scale, out=out[:mm])
        if mm == M:
            return out
        parts, kk = 8, K // 8
        P = self._buf("splitk_P", (parts, M - mm, N), torch.float32)
        ops.gemm_grouped([(a[mm:, i * kk:(i + 1) * kk], w[:, i * kk:(i + 1) * kk], P[i]) for i in range(parts)])
        ops.splitk_fixup(P, out[mm:], "relu_dropout" if y is None else "drelu", bias=bias,
                         residual=None if y is None else y[mm:], row0=mm, seed=seed, p=self.p, scale=scale)
        return out

    def W(self, i: int) -> torch.Tensor:
        return self.cviews[f"linear{i}.weight"]

    def b(self, i: int) -> Optional[torch.Tensor]:
        return self.views.get(f"linear{i}.bias")

    def layer_seed(self, layer: int) -> int:
        """Dropout stream of one forward layer in the current step."""
        return (self.seed * 1_000_003 + self.step_count * 7919 + layer * 104_729) & (2**64 - 1)

    def flops_per_step(self, Hs: int) -> float:
        """MFMA FLOPs of one step (forward + data-grad + weight-grad GEMMs)."""
        Hp = _pad64(Hs)
        fwd = 2.0 * Hp * (D * H + H * H + H * D + D * H + H * D)
        return 3.0 * fwd

    def hbm_bytes_per_step(self, Hs: int, U: int) -> dict:
        """Algorithmic HBM bytes of the step's non-GEMM kernels (the GEMMs are
        priced by their FLOPs): AdamW 30 B per parameter (f32 param, grad, m, v
        read; param, m, v written; the bf16 mirror written) and the row kernels
        per history slot (es = 2 bf16): slots_kernel reads the token row and
        writes S and XH (2 D es), pool fwd reads (X, P) (2 D es), pool bwd reads
        them again and writes dXp and dL (4 D es) -- 8 D es per slot -- plus the
        four weight transposes read and written once (W5, W4, W3: D H each;
        W2: H H)."""
        es = 2 if self.dtype == torch.bfloat16 else 4
        Hp = _pad64(Hs)
        rows = Hp * 8 * D * es + U * D * 2 + 2 * es * (3 * D * H + H * H)
        return {"adamw": 30.0 * self.n_flat, "row_kernels": float(rows)}


class LatentAttentionTrainStep(_FlatTrainStep):
    """Config-5 step with ``LatentAttentionModel`` in the pooler slot (BASELINE
    configs[4]: "backward for encoder + latent attention"; the reference
    trainer's loop, trainer.py:1044-1069, with the latent pooler) as ONE library
    call per batch (``nr_latent_train_step``, csrc/latent_train.hip):

      E     = g_mlp_LN(last token of each unique news)
      fold  K/V of the 64 latents into A (scores) and Bt (output) once per step
      per history slot: X = LN_q(E[hist]); P = softmax64(X Aᵀ); H1 = P Btᵀ + E[hist];
                        Z = GEGLU(LN_f(H1) W1ᵀ + b1)
      per batch row:    m = mean(Z) W2ᵀ + b2 + mean(H1)  (the last linear layer commutes
                        with the history mean: its three GEMMs run over B rows, not slots)
      users = normalize(m); loss = MarginRankingLoss(2)(cos(users, E[pos]), cos(users, E[neg]))
      backward of all of it; clip_grad_norm_(0.5) + AdamW   (grad norm in the step), nr_adamw

    dtype float32: exact-f32 MFMA GEMMs and f32 activations (the parity mode);
    bfloat16: bf16 operands and activations with f32 accumulation, statistics
    and gradients, weights read from a bf16 mirror AdamW rewrites."""

    _what, _prefix = "latent-attention train step", "latent."
    _args, _step_fn, _workspace_fn = _lib.LatentTrainArgs, "nr_latent_train_step", "nr_latent_train_workspace_bytes"
    _contrastive_fn = "nr_latent_train_step_contrastive"
    _pmap = {"tok_g": "ln.weight", "tok_b": "ln.bias", "latents": "latent.latents",
             "nq_g": _BLK + "0.norm.weight", "nq_b": _BLK + "0.norm.bias",
             "nc_g": _BLK + "0.norm_context.weight", "nc_b": _BLK + "0.norm_context.bias",
             "Wq": _BLK + "0.fn.to_q.weight", "Wkv": _BLK + "0.fn.to_kv.weight", "Wo": _BLK + "0.fn.to_out.weight",
             "nf_g": _BLK + "1.norm.weight", "nf_b": _BLK + "1.norm.bias",
             "W1": _BLK + "1.fn.net.0.weight", "b1": _BLK + "1.fn.net.0.bias",
             "W2": _BLK + "1.fn.net.2.weight", "b2": _BLK + "1.fn.net.2.bias"}
    _mirrored = ("Wq", "Wkv", "Wo", "W1", "W2")

    def __init__(self, token_model, latent_model, dtype: torch.dtype = torch.float32, lr: float = 1e-6,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, max_norm: float = 0.5,
                 seed: int = 1234, device=None, temperature: float = 1.0):
        # (no dropout argument: LatentAttentionModel has no dropout, latent_attention.py:77-171)
        super().__init__(token_model, latent_model, dtype, lr, betas, eps, weight_decay, max_norm, seed, device,
                         temperature)
        self.model = latent_model
        if abs(self.ln_eps - 1e-12) > 1e-18:
            raise NewsRecHIPError("the token LayerNorm of MyLayer has eps 1e-12 (attention.py:155)")
        if set(self._pmap.values()) != set(self.names):
            raise NewsRecHIPError(f"unexpected LatentAttentionModel parameters: {sorted(self.names)}")

    def flops_per_step(self, Hs: int, B: int = 256) -> float:
        """MFMA FLOPs the step executes (forward, data-grad and weight-grad GEMMs,
        the fold and its backward; the last layer's GEMMs over B rows)."""
        Hp, Bp = _pad64(Hs), _pad64(B)
        slot = 2.0 * Hp * (D * 512 + 512 * D + D * 8192)          # P, H1, G
        row = 2.0 * Bp * 4096 * D                                  # m = mean(Z) W2^T
        fold = 2.0 * 64 * D * 8192 + 2 * (2.0 * 8 * 64 * 512 * D)  # KV, A, Bt^T
        return 3.0 * (slot + row + fold)

    def hbm_bytes_per_step(self, Hs: int, U: int) -> dict:
        """Algorithmic HBM bytes of the step's non-GEMM kernels: AdamW as in
        FinalAttentionTrainStep, and the row kernels per history slot (es = 2 bf16):
        gather + LN_q writes S and X (2 D es); segmean reads G and H1 (8192 es + D es);
        the GEGLU backward reads G and writes dG (2 x 8192 es); the LN_f backward reads
        H1 and dY and writes dH1 (3 D es); the LN_q backward reads dX and X and adds dE in
        f32 (2 D es + 4 D) -- 32,768 es + 4 D bytes per slot -- plus the token rows read."""
        es = 2 if self.dtype == torch.bfloat16 else 4
        Hp = _pad64(Hs)
        per_slot = (2 * D + 8192 + D + 2 * 8192 + 3 * D + 2 * D) * es + 4 * D
        return {"adamw": 30.0 * self.n_flat, "row_kernels": float(Hp * per_slot + U * D * 2)}

    def model_flops_per_step(self, Hs: int) -> float:
        """The reference formulation's GEMM FLOPs (every linear layer per history
        slot, K/V once): what rounds 1-3 reported as this step's gemm_tflops."""
        Hp = _pad64(Hs)
        return 3.0 * 2.0 * Hp * (D * 512 + 512 * D + D * 8192 + 4096 * D)
