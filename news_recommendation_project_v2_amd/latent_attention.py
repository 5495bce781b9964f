"""Perceiver-style latent-attention history pooler (reference latent_attention.py).

Parameter names match the reference module (latent_attention.py:115-131), so a
reference state_dict loads unchanged:
  latents [64, 1024]
  cross_attend_blocks.0.{norm, norm_context}.{weight, bias}
  cross_attend_blocks.0.fn.{to_q [4096,1024], to_kv [8192,1024], to_out [1024,4096]}.weight
  cross_attend_blocks.1.norm.{weight, bias}
  cross_attend_blocks.1.fn.net.0.{weight [8192,1024], bias}, .net.2.{weight [1024,4096], bias}

MI355X formulation.  Every history item attends to the SAME 64 latents, so the
keys/values depend only on the weights (latent_attention.py:161-162 rebuilds
them for every batch row).  They are computed once per model and folded into
the query and output projections:
  scores_h = LN_q(e) W_q,hᵀ K_hᵀ / sqrt(512) = LN_q(e) · A_hᵀ,   A_h  = K_h W_q,h / sqrt(512)
  out      = sum_h W_o,h (P_h V_h)            = P · Btᵀ,        Bt[:, h*64+j] = W_o,h V_h[j]
which turns the 1024->4096 query and 4096->1024 output projections (16.8
MFLOP/item) into 1024->512 and 512->1024 GEMMs (2.1 MFLOP/item), exact up to
f32 rounding.  The fold is done once in float64 on the host (a weight loader
step, like reading a checkpoint), then moved to the device.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from ._lib import NewsRecHIPError
from .config import (EMBEDDING_DIM, LATENT_CROSS_DIM_HEAD, LATENT_CROSS_HEADS, LATENT_FF_MULT,
                     LATENT_NUM_LATENTS, REDUCED_DIM)


class PreNorm(torch.nn.Module):
    """LayerNorm on the input (and on the context when context_dim is given)."""

    def __init__(self, dim: int, fn: torch.nn.Module, context_dim: Optional[int] = None):
        super().__init__()
        self.fn = fn
        self.norm = torch.nn.LayerNorm(dim)
        self.norm_context = torch.nn.LayerNorm(context_dim) if context_dim is not None else None


class GEGLU(torch.nn.Module):
    """a * gelu(g) over the two halves of the last dim (latent_attention.py:24-27)."""


class FeedForward(torch.nn.Module):
    def __init__(self, dim: int, mult: int = 4):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(dim, dim * mult * 2), GEGLU(),
                                       torch.nn.Linear(dim * mult, dim))


class Attention(torch.nn.Module):
    def __init__(self, query_dim: int, context_dim: Optional[int] = None, heads: int = 8, dim_head: int = 64):
        super().__init__()
        inner = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.to_q = torch.nn.Linear(query_dim, inner, bias=False)
        self.to_kv = torch.nn.Linear(context_dim, inner * 2, bias=False)
        self.to_out = torch.nn.Linear(inner, query_dim, bias=False)


def interleave_geglu_rows(w: torch.Tensor, block: int = 32) -> torch.Tensor:
    """[2F, ...] with rows (a_0..a_F-1, g_0..g_F-1) -> 32-row blocks (a, g, a, g, ...)
    so one 64-column GEMM tile holds matching a/g columns (NR_EPI_GEGLU)."""
    two_f = w.shape[0]
    f = two_f // 2
    a = w[:f].reshape(f // block, block, *w.shape[1:])
    g = w[f:].reshape(f // block, block, *w.shape[1:])
    return torch.stack([a, g], dim=1).reshape(two_f, *w.shape[1:])


def lnfold_weights(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor],
                   tag: str) -> Dict[str, torch.Tensor]:
    """Weights that apply LayerNorm(gamma, beta) inside the GEMM that consumes it
    (nr_latent_transform_lnfold, bf16): for a row a with LN stats (mean, rstd),
        LN(a) . w_n + b_n = rstd (a . w'_n - mean u_n) + c_n,
        w' = w o gamma (rounded to bf16),  u_n = sum_k w'_nk,  c_n = beta . w_n + b_n,
    u taken from the ROUNDED w' (float64 sums) so a constant row maps exactly to c.
    Returns {"W<tag>": bf16 [N, K], "uc<tag>": f32 [2, N]}."""
    w64 = w.to(torch.float64)
    wf = (w64 * gamma.to(torch.float64)[None, :]).to(torch.bfloat16)
    u = wf.to(torch.float64).sum(1)
    c = w64 @ beta.to(torch.float64)
    if bias is not None:
        c = c + bias.to(torch.float64)
    return {f"W{tag}_ln": wf.contiguous(), f"uc{tag}": torch.stack([u, c]).to(torch.float32).contiguous()}


def _param_key(module: torch.nn.Module, dtype) -> tuple:
    """Cache key of a pooler's prepared device weights: dtype, device, and every
    parameter's storage and version (an in-place edit or a re-pointed ``.data``
    moves it; writes through raw pointers do not -- the train steps reset the cache)."""
    ps = list(module.parameters())
    return (dtype, ps[0].device, tuple((p.data_ptr(), p._version) for p in ps))


class _LatentItemFn(torch.autograd.Function):
    """Per-item hiddens of LatentAttentionModel (latent_attention.py:157-163) with
    their backward on the HIP kernels, over packed
    valid rows padded with zeros to a multiple of 64 (the weight-grad GEMMs' K):

      X  = LN_q(E)                          nr_layernorm
      P  = softmax64(X Aᵀ)                  nr_gemm SOFTMAX64   (A = the folded K·W_q / √512, [512, D])
      H1 = P Btᵀ + E                        nr_gemm RESADD      (Bt = the folded W_o·Vᵀ, [D, 512])
      Y  = LN_f(H1);  G = Y W1ᵀ + b1        nr_layernorm, nr_gemm
      Z  = a ⊙ gelu(g), (a, g) = G.chunk(2) nr_geglu_fwd
      H  = Z W2ᵀ + b2 + H1                  nr_gemm RESADD

    Backward: data grads through transposed weights (nr_transpose + nr_gemm),
    nr_geglu_bwd, nr_softmax64_bwd, nr_layernorm_bwd (the residual grads added
    in the same pass), weight grads dOutᵀ·In as one grouped GEMM, bias and LN
    parameter grads by column sums / nr_ln_param_grad.  A and Bt are built from
    the module's parameters by differentiable torch ops (LatentAttentionModel.
    _fold_train: 64-latent weight algebra, the reference's own to_kv(latents)),
    so autograd carries dA and dBt on to latents, norm_context, to_q, to_kv and
    to_out.  The padding rows carry zero gradient.  GEMM operands are f32 (exact-f32
    MFMA, the module API's default) or, with ``mm_dtype=bfloat16`` (the config-5
    train step's bf16 mode), bf16 with f32 accumulation and f32 outputs."""

    @staticmethod
    def forward(ctx, rows, A, Bt, gq, bq, gf, bf, W1, b1, W2, b2, mm_dtype=torch.float32):
        Hs = rows.shape[0]
        E = ops.padded_rows(rows)
        A, Bt, W1, W2 = A.contiguous(), Bt.contiguous(), W1.contiguous(), W2.contiguous()
        f32 = torch.float32
        # GEMM operands in mm_dtype (bf16: MFMA bf16 operands, f32 accumulate and f32
        # outputs -- the LN / softmax / GEGLU kernels and the residual stream stay f32)
        c = (lambda t: t) if mm_dtype == f32 else (lambda t: ops.gather_rows(t, None, out_dtype=mm_dtype))
        # X, Y, Z feed only GEMMs (here and as weight-grad operands): written in mm_dtype
        X = ops.layernorm(E, gq.contiguous(), bq.contiguous(), 1e-5, out_dtype=mm_dtype)
        P = ops.gemm(X, c(A), None, epilogue="softmax64", out_dtype=f32)
        H1 = ops.gemm(c(P), c(Bt), None, epilogue="resadd", residual=E, out_dtype=f32)
        Y = ops.layernorm(H1, gf.contiguous(), bf.contiguous(), 1e-5, out_dtype=mm_dtype)
        G = ops.gemm(Y, c(W1), b1.contiguous(), out_dtype=f32)
        Z = ops.geglu_fwd(G, out_dtype=mm_dtype)
        H = ops.gemm(Z, c(W2), b2.contiguous(), epilogue="resadd", residual=H1, out_dtype=f32)
        ctx.save_for_backward(E, X, P, H1, Y, G, Z, A, Bt, gq, gf, W1, W2)
        ctx.Hs, ctx.mm_dtype = Hs, mm_dtype
        return H[:Hs]

    @staticmethod
    def backward(ctx, dH):
        E, X, P, H1, Y, G, Z, A, Bt, gq, gf, W1, W2 = ctx.saved_tensors
        Hs, lo = ctx.Hs, ctx.mm_dtype
        D, dev = E.shape[1], E.device
        f32 = torch.float32
        dHp = ops.padded_rows(dH)
        c = (lambda t: t) if lo == f32 else (lambda t: ops.gather_rows(t, None, out_dtype=lo))
        T = lambda t: ops.transpose(t, out_dtype=lo)
        dZ = ops.gemm(c(dHp), T(W2), out_dtype=f32)
        dG = ops.geglu_bwd(G, dZ, out_dtype=lo)  # feeds GEMMs and the b1 column sum only
        dY = ops.gemm(dG, T(W1), out_dtype=f32)
        dH1 = ops.layernorm_bwd(H1, gf.contiguous(), dY, 1e-5, residual=dHp)
        dP = ops.gemm(c(dH1), T(Bt), out_dtype=f32)
        dS = ops.softmax64_bwd(P, dP, out_dtype=lo)
        dX = ops.gemm(dS, T(A), out_dtype=f32)
        dE = ops.layernorm_bwd(E, gq.contiguous(), dX, 1e-5, residual=dH1)
        gW2 = torch.empty(W2.shape, dtype=f32, device=dev)
        gW1 = torch.empty(W1.shape, dtype=f32, device=dev)
        gBt = torch.empty(Bt.shape, dtype=f32, device=dev)
        gA = torch.empty(A.shape, dtype=f32, device=dev)
        ops.gemm_grouped([(T(dHp), T(Z), gW2), (T(dG), T(Y), gW1), (T(dH1), T(P), gBt), (T(dS), T(X), gA)])
        gb2 = torch.zeros(D, dtype=torch.float32, device=dev)
        gb1 = torch.zeros(W1.shape[0], dtype=torch.float32, device=dev)
        ops.col_sum(dHp, gb2)
        ops.col_sum(dG, gb1)
        ggf, gbf, ggq, gbq = (torch.zeros(D, dtype=torch.float32, device=dev) for _ in range(4))
        ops.ln_param_grad(H1, None, 1e-5, dY, ggf, gbf)
        ops.ln_param_grad(E, None, 1e-5, dX, ggq, gbq)
        return dE[:Hs], gA, gBt, ggq, gbq, ggf, gbf, gW1, gb1, gW2, gb2, None


class _SegmentMeanFn(torch.autograd.Function):
    """Masked mean over each batch row's valid items (latent_attention.py:166-168)
    on the packed rows: forward is the pooling kernel's mean pass (nr_pool_score
    pooling-only, NR_POOL_MEAN: one wave per segment, fixed summation order, so
    the result is deterministic, unlike an atomic index_add); backward spreads
    du / count back over the segment's rows.  An empty segment gives 0/0 = NaN,
    as the reference's s / d does."""

    @staticmethod
    def forward(ctx, H, off):
        ctx.save_for_backward(off)
        ctx.n_rows = H.shape[0]
        return ops.pool_rows("mean", H.contiguous(), off)

    @staticmethod
    def backward(ctx, du):
        (off,) = ctx.saved_tensors
        counts = off[1:] - off[:-1]
        per_row = (du / counts.unsqueeze(1).to(du.dtype)).repeat_interleave(counts, dim=0, output_size=ctx.n_rows)
        return per_row, None


def segment_mean(H: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    return _SegmentMeanFn.apply(H, off)


class LatentAttentionModel(torch.nn.Module):
    """forward(embeddings [B, L, D], attention_mask [B, L] | None).

    mask given : [B, D] = normalize(masked mean over L of the per-item hiddens)
    mask None  : [B, L, D] per-item hiddens (latent_attention.py:165)
    """

    pooler_kind = "latent"

    def __init__(self):
        super().__init__()
        if EMBEDDING_DIM != 1024:
            # the reference's EMBEDDING_DIM == 4096 branch (latent_attention.py:91-97: 32
            # latents, 2 heads of 32, the NV-Embed experiment) is out of scope:
            # nr_pool_score and the transforms are built for D = 1024 only, so refuse here
            # rather than construct a model every kernel would reject
            raise NotImplementedError(f"LatentAttentionModel: EMBEDDING_DIM={EMBEDDING_DIM}; the HIP path "
                                      "supports 1024 (the e5-large-instruct / XLM-R-large width) only")
        num_latents, latent_dim, heads, dim_head = (LATENT_NUM_LATENTS, REDUCED_DIM, LATENT_CROSS_HEADS,
                                                    LATENT_CROSS_DIM_HEAD)
        dim = REDUCED_DIM
        self.cross_attend_blocks = torch.nn.ModuleList([
            PreNorm(latent_dim, Attention(latent_dim, dim, heads=heads, dim_head=dim_head), context_dim=dim),
            PreNorm(latent_dim, FeedForward(latent_dim, mult=LATENT_FF_MULT)),
        ])
        self.output_normalize = True
        self.latents = torch.nn.Parameter(torch.randn(num_latents, latent_dim))
        self._hip_cache: Dict[tuple, dict] = {}

    @torch.no_grad()
    def folded_weights(self) -> Dict[str, torch.Tensor]:
        """float64 host fold of the constant latent K/V into A and Bt (see module doc)."""
        attn_blk, ff_blk = self.cross_attend_blocks
        attn = attn_blk.fn
        h = attn.heads
        d64 = lambda t: t.detach().to("cpu", torch.float64)
        lat = d64(self.latents)
        lat_n = torch.nn.functional.layer_norm(lat, lat.shape[-1:], d64(attn_blk.norm_context.weight),
                                               d64(attn_blk.norm_context.bias), attn_blk.norm_context.eps)
        kv = lat_n @ d64(attn.to_kv.weight).T                # [nl, 2*inner]
        inner = kv.shape[1] // 2
        dh = inner // h
        k, v = kv[:, :inner], kv[:, inner:]
        wq = d64(attn.to_q.weight)                         # [inner, D]
        wo = d64(attn.to_out.weight)                       # [D, inner]
        scale = 1.0 / math.sqrt(dh)                        # SDPA default scale
        a_blocks, bt_blocks = [], []
        for hh in range(h):
            sl = slice(hh * dh, (hh + 1) * dh)
            a_blocks.append((k[:, sl] @ wq[sl, :]) * scale)   # [nl, D]
            bt_blocks.append(wo[:, sl] @ v[:, sl].T)          # [D, nl]
        ff = ff_blk.fn.net
        return {
            "A": torch.cat(a_blocks, 0),
            "Bt": torch.cat(bt_blocks, 1),
            "W1i": interleave_geglu_rows(d64(ff[0].weight)),
            "b1i": interleave_geglu_rows(d64(ff[0].bias)),
            "W2": d64(ff[2].weight),
            "b2": d64(ff[2].bias),
            "lnq_g": d64(attn_blk.norm.weight), "lnq_b": d64(attn_blk.norm.bias),
            "lnf_g": d64(ff_blk.norm.weight), "lnf_b": d64(ff_blk.norm.bias),
        }

    def hip_weights(self, dtype: torch.dtype = torch.float32) -> dict:
        key = _param_key(self, dtype)
        w = self._hip_cache.get(key)
        if w is None:
            dev = self.latents.device
            fw = self.folded_weights()
            w = {}
            for name, t in fw.items():
                tgt = dtype if name in ("A", "Bt", "W1i", "W2") else torch.float32
                w[name] = t.to(tgt).to(dev).contiguous()
            if dtype == torch.bfloat16:
                for name, t in lnfold_weights(fw["A"], fw["lnq_g"], fw["lnq_b"], None, "q").items():
                    w[name] = t.to(dev).contiguous()
                for name, t in lnfold_weights(fw["W1i"], fw["lnf_g"], fw["lnf_b"], fw["b1i"], "f").items():
                    w[name] = t.to(dev).contiguous()
            self._hip_cache = {key: w}
        return w

    def item_table(self, rows: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """Per-item hiddens [n, D] for rows [n, D] (one per unique news)."""
        dtype = dtype or rows.dtype
        return ops.latent_transform(rows.to(dtype).contiguous(), self.hip_weights(dtype))

    def _fold_train(self):
        """A [h*64, D] and Bt [D, h*64] of the fold (module doc) as differentiable
        f32 device ops on the parameters: the reference's to_kv(LN_c(latents))
        (latent_attention.py:161-162) once per batch instead of once per row."""
        attn_blk = self.cross_attend_blocks[0]
        attn = attn_blk.fn
        h = attn.heads
        lat_n = torch.nn.functional.layer_norm(self.latents, self.latents.shape[-1:], attn_blk.norm_context.weight,
                                               attn_blk.norm_context.bias, attn_blk.norm_context.eps)
        kv = lat_n @ attn.to_kv.weight.T                              # [nl, 2 inner]
        inner = kv.shape[1] // 2
        dh = inner // h
        nl, d = self.latents.shape[0], attn.to_q.weight.shape[1]
        k = kv[:, :inner].reshape(nl, h, dh).permute(1, 0, 2)        # [h, nl, dh]
        v = kv[:, inner:].reshape(nl, h, dh).permute(1, 2, 0)        # [h, dh, nl]
        a = torch.matmul(k, attn.to_q.weight.reshape(h, dh, d)) * (1.0 / math.sqrt(dh))   # [h, nl, D]
        bt = torch.matmul(attn.to_out.weight.reshape(d, h, dh).permute(1, 0, 2), v)      # [h, D, nl]
        return a.reshape(h * nl, d), bt.permute(1, 0, 2).reshape(d, h * nl)

    def _train_items(self, rows: torch.Tensor, mm_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        params = list(self.parameters())
        if any(p.dtype != torch.float32 for p in params):
            raise NewsRecHIPError("LatentAttentionModel autograd path trains f32 parameters (as the reference does)")
        attn_blk, ff_blk = self.cross_attend_blocks
        A, Bt = self._fold_train()
        ff = ff_blk.fn.net
        return _LatentItemFn.apply(rows.float(), A, Bt, attn_blk.norm.weight, attn_blk.norm.bias, ff_blk.norm.weight,
                                   ff_blk.norm.bias, ff[0].weight, ff[0].bias, ff[2].weight, ff[2].bias, mm_dtype)

    def forward(self, embeddings: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if embeddings.device.type != "cuda":
            raise NewsRecHIPError("LatentAttentionModel.forward runs on the MI355X HIP path only (got a CPU tensor)")
        b, l, d = embeddings.shape
        train = self.training or (torch.is_grad_enabled() and (embeddings.requires_grad or
                                                               any(p.requires_grad for p in self.parameters())))
        if attention_mask is None:
            rows = embeddings.reshape(b * l, d)
            table = self._train_items(rows) if train else self.item_table(rows.float())
            return table.reshape(b, l, d)
        from .modeling_utils import flatten_valid, pool_rows
        rows, off = flatten_valid(embeddings, attention_mask)
        if not train:
            return pool_rows("latent", self.item_table(rows.float()), off)
        # autograd: per-item hiddens on the HIP kernels, then the reference's masked mean
        # and F.normalize (latent_attention.py:166-170) on the [B, D] users
        u = segment_mean(self._train_items(rows), off)
        return torch.nn.functional.normalize(u, p=2, dim=-1) if self.output_normalize else u


def exists(val):
    """latent_attention.py:43-44."""
    return val is not None


def default(val, d):
    """latent_attention.py:47-48."""
    return val if exists(val) else d
