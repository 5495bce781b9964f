"""Tensor-level wrappers over the C-ABI (include/newsrec.h).

Every function takes device tensors (PyTorch-ROCm "cuda" tensors), validates
shapes/dtypes/strides on the host, and enqueues the HIP kernel on the current
torch stream.  There is no CPU fallback: non-device tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib

_DT = {torch.float32: _lib.NR_F32, torch.bfloat16: _lib.NR_BF16}
# dtypes of the token-state rows (the blobs are fp16): gather_layernorm, ln_param_grad, the train steps
TOKEN_DT = {**_DT, torch.float16: _lib.NR_F16}
_EPI = {
    "none": _lib.NR_EPI_NONE,
    "relu": _lib.NR_EPI_RELU,
    "exp": _lib.NR_EPI_EXP,
    "geglu": _lib.NR_EPI_GEGLU,
    "resadd": _lib.NR_EPI_RESADD,
    "gelu": _lib.NR_EPI_GELU,
    "softmax64": _lib.NR_EPI_SOFTMAX64,
    "softmax64_bwd": _lib.NR_EPI_SOFTMAX64_BWD,  # residual = the softmax output P
}
POOLERS = {"final": _lib.NR_POOL_FINAL, "latent": _lib.NR_POOL_LATENT, "mean": _lib.NR_POOL_MEAN}


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise _lib.NewsRecHIPError(
                f"HIP kernels need device tensors, got a tensor on {t.device} (no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise _lib.NewsRecHIPError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _rowmajor(t: torch.Tensor, name: str) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.NewsRecHIPError(f"{name} must be a row-major 2-D tensor (stride(1)==1)")
    return t.stride(0)


def _dtype(t: torch.Tensor, name: str) -> int:
    if t.dtype not in _DT:
        raise _lib.NewsRecHIPError(f"{name}: unsupported dtype {t.dtype}")
    return _DT[t.dtype]


def _pad64(n: int) -> int:
    """Rows padded to a multiple of 64 (the weight-grad GEMMs' K), at least 64."""
    return max(64, (n + 63) // 64 * 64)


def padded_rows(rows: torch.Tensor) -> torch.Tensor:
    """``rows`` [n, D] as a fresh f32 [_pad64(n), D] tensor, the padding rows zero."""
    n = rows.shape[0]
    out = torch.empty((_pad64(n), rows.shape[1]), dtype=torch.float32, device=rows.device)
    out[:n] = rows
    out[n:].zero_()
    return out


def grow_workspace(ws: Optional[torch.Tensor], need: int, dev) -> torch.Tensor:
    """``ws`` when it holds ``need`` bytes, else a new uint8 buffer of that size
    (callers keep the result, so a workspace only ever grows)."""
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def set_persistent_workgroups(n: int = 0) -> None:
    """Workgroups of the persistent bf16 GEMM launches (0 = one per CU): set it
    to the CU count of a CU-masked stream the transform runs on."""
    _lib.call("nr_set_persistent_workgroups", int(n))


def persistent_workgroups() -> int:
    """The current persistent-GEMM workgroup budget (0 = one per CU)."""
    return int(_lib.load().nr_persistent_workgroups())


def set_gemm_half_tail(on: bool = True) -> None:
    """Half-tile tail of the persistent bf16 GEMM (default on; bit-identical
    either way -- the switch is for A/B timing)."""
    _lib.call("nr_set_gemm_half_tail", int(bool(on)))


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
         epilogue: str = "none", residual: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """out = epilogue(a @ w.T + bias [+ residual]); w in nn.Linear layout [N, K]."""
    dev = _dev(a, w, bias, residual, out)
    if a.dtype != w.dtype:
        raise _lib.NewsRecHIPError("gemm: a and w must share a dtype")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.NewsRecHIPError(f"gemm: K mismatch {K} vs {K2}")
    epi = _EPI[epilogue]
    ncols = N // 2 if epilogue == "geglu" else N
    if out is None:
        out = torch.empty((M, ncols), dtype=out_dtype or a.dtype, device=dev)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != N):
        raise _lib.NewsRecHIPError("gemm: bias must be contiguous f32 [N]")
    if residual is not None and residual.dtype != out.dtype:
        raise _lib.NewsRecHIPError("gemm: residual must have the output dtype")
    if out.shape != (M, ncols):
        raise _lib.NewsRecHIPError(f"gemm: out shape {tuple(out.shape)} != {(M, ncols)}")
    lda, ldw, ldc = _rowmajor(a, "a"), _rowmajor(w, "w"), _rowmajor(out, "out")
    ldr = _rowmajor(residual, "residual") if residual is not None else 0
    _lib.call("nr_gemm", _dtype(a, "a"), _dtype(out, "out"), epi, M, N, K, _ptr(a), lda, _ptr(w), ldw,
              _ptr(bias), _ptr(residual), ldr, _ptr(out), ldc, _stream(dev))
    return out


def layernorm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
              out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    dev = _dev(x, gamma, beta, out)
    rows, dim = x.shape
    if out is None:
        out = torch.empty((rows, dim), dtype=out_dtype or x.dtype, device=dev)
    _lib.call("nr_layernorm", _dtype(x, "x"), _dtype(out, "out"), rows, dim, _ptr(x), _rowmajor(x, "x"),
              _ptr(gamma), _ptr(beta), ctypes.c_float(eps), _ptr(out), _rowmajor(out, "out"), _stream(dev))
    return out


def gather_layernorm(x: torch.Tensor, row_idx: Optional[torch.Tensor], gammas: Optional[torch.Tensor],
                     betas: Optional[torch.Tensor], eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = LN chain (gammas/betas [n_ln, D]) of x[row_idx[i]] (identity if None), f32 out.

    x may be f32, bf16 or f16 (the token-state blobs are fp16)."""
    dev = _dev(x, row_idx, gammas, betas, out)
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.NewsRecHIPError("gather_layernorm: x must be row-major 2-D")
    dt = TOKEN_DT.get(x.dtype)
    if dt is None:
        raise _lib.NewsRecHIPError(f"gather_layernorm: unsupported dtype {x.dtype}")
    dim = x.shape[1]
    if row_idx is not None:
        if row_idx.dtype != torch.int64 or not row_idx.is_contiguous():
            raise _lib.NewsRecHIPError("gather_layernorm: row_idx must be contiguous int64")
        n = row_idx.numel()
    else:
        n = x.shape[0]
    n_ln = 0
    for t in (gammas, betas):
        if t is not None:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != dim:
                raise _lib.NewsRecHIPError("gather_layernorm: gammas/betas must be contiguous f32 [n_ln, D]")
            n_ln = max(n_ln, t.shape[0])
    if gammas is not None and betas is not None and gammas.shape != betas.shape:
        raise _lib.NewsRecHIPError("gather_layernorm: gammas and betas differ in shape")
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.shape != (n, dim):
        raise _lib.NewsRecHIPError("gather_layernorm: out must be f32 [n, D]")
    _lib.call("nr_gather_layernorm", dt, n, dim, _ptr(x), x.stride(0), _ptr(row_idx), n_ln, _ptr(gammas),
              _ptr(betas), ctypes.c_float(eps), _ptr(out), _rowmajor(out, "out"), _stream(dev))
    return out


def softmax64(x: torch.Tensor, out: Optional[torch.Tensor] = None,
              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    dev = _dev(x, out)
    if x.dtype != torch.float32:
        raise _lib.NewsRecHIPError("softmax64: x must be f32")
    rows, width = x.shape
    if width % 64:
        raise _lib.NewsRecHIPError("softmax64: width must be a multiple of 64")
    if out is None:
        out = torch.empty((rows, width), dtype=out_dtype or torch.float32, device=dev)
    _lib.call("nr_softmax64", rows, width // 64, _ptr(x), _rowmajor(x, "x"), _dtype(out, "out"), _ptr(out),
              _rowmajor(out, "out"), _stream(dev))
    return out


def row_inv_norm(x: torch.Tensor, eps: float = 1e-8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1 / max(||x_r||, eps) per row, f32 (cosine_similarity's per-vector clamp)."""
    dev = _dev(x, out)
    rows, dim = x.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=dev)
    _lib.call("nr_row_inv_norm", _dtype(x, "x"), rows, dim, _ptr(x), _rowmajor(x, "x"), ctypes.c_float(eps),
              _ptr(out), _stream(dev))
    return out


def row_stats(x: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row LayerNorm statistics [rows, 2] f32 = (mean, 1/sqrt(biased var + eps))."""
    dev = _dev(x, out)
    rows, dim = x.shape
    if out is None:
        out = torch.empty((rows, 2), dtype=torch.float32, device=dev)
    _lib.call("nr_row_stats", _dtype(x, "x"), rows, dim, _ptr(x), _rowmajor(x, "x"), ctypes.c_float(eps),
              _ptr(out), _stream(dev))
    return out


def _check_csr(idx: torch.Tensor, off: torch.Tensor, name: str) -> None:
    if idx.dtype != torch.int32 or not idx.is_contiguous():
        raise _lib.NewsRecHIPError(f"{name}_idx must be contiguous int32")
    if off.dtype != torch.int64 or not off.is_contiguous():
        raise _lib.NewsRecHIPError(f"{name}_off must be contiguous int64")


def _check_inv_norm(cand_inv_norm: torch.Tensor, n_news: int, contiguous: bool = True) -> None:
    if (cand_inv_norm.dtype != torch.float32 or cand_inv_norm.numel() < n_news
            or (contiguous and not cand_inv_norm.is_contiguous())):
        raise _lib.NewsRecHIPError(f"cand_inv_norm must be {'contiguous ' if contiguous else ''}f32 with one entry per "
                                   "candidate-table row")


def _check_scan(what: str, users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
                excl_idx: Optional[torch.Tensor], excl_off: Optional[torch.Tensor], check_rows: bool = True):
    """Host checks of a scan of the whole table (topk_users, rank_targets): returns (n_users,
    dim, n_news, ld, dt, excl_idx), the exclusion rows range-checked (one small sync; not
    without ``check_rows``: a pager's later calls with the lists of its first) and an empty
    list replaced by a one-slot dummy."""
    if users.dtype != torch.float32 or users.dim() != 2 or not users.is_contiguous():
        raise _lib.NewsRecHIPError(f"{what}: users must be contiguous f32 [U, D]")
    n_users, dim = users.shape
    n_news = cand_table.shape[0]
    ld = _rowmajor(cand_table, "cand_table")
    if cand_table.shape[1] != dim:
        raise _lib.NewsRecHIPError(f"{what}: users and cand_table must share their width")
    _check_inv_norm(cand_inv_norm, n_news)
    if (excl_idx is None) != (excl_off is None):
        raise _lib.NewsRecHIPError(f"{what}: excl_idx and excl_off go together")
    if excl_idx is not None:
        _check_csr(excl_idx, excl_off, "excl")
        if excl_off.numel() != n_users + 1:
            raise _lib.NewsRecHIPError(f"{what}: excl_off must have U + 1 entries")
        if excl_idx.numel() and check_rows:
            lo, hi = (int(v) for v in torch.aminmax(excl_idx))
            if lo < 0 or hi >= n_news:
                raise IndexError(f"{what}: excluded row {lo if lo < 0 else hi} is outside the {n_news} table rows")
        elif not excl_idx.numel():  # no storage behind an empty tensor; the kernel never reads it
            excl_idx = torch.zeros(1, dtype=torch.int32, device=users.device)
    return n_users, dim, n_news, ld, _dtype(cand_table, "cand_table"), excl_idx


def _outputs(what: str, spec, out, dev, real_slots: bool = False):
    """The optional outputs of ``what``: ``spec`` = (name, dtype, shape, wanted) per output,
    ``out`` = the caller's tuple (None: allocate the wanted ones).  Returns (bufs, res): one
    tensor or None per output for the call, and the wanted ones to return.  ``real_slots``
    puts a real (unwritten) slot behind a zero-element tensor, whose data_ptr() is 0."""
    if out is None:
        out = tuple(torch.empty(shape, dtype=dtype, device=dev) if want else None for _, dtype, shape, want in spec)
    elif len(out) != len(spec):
        raise _lib.NewsRecHIPError(f"{what}: out must be ({', '.join(name for name, *_ in spec)}), None for the ones "
                                   "not wanted")
    for t, (name, dtype, shape, want) in zip(out, spec):
        if want and t is None:
            raise _lib.NewsRecHIPError(f"{what}: out has no {name}")
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.NewsRecHIPError(f"{what}: out {name} must be contiguous {dtype} of shape {shape}")
    res = tuple(t for t, (_, _, _, want) in zip(out, spec) if want)
    if real_slots:
        out = [t if t is None or t.numel() else torch.empty(1, dtype=t.dtype, device=dev) for t in out]
    return out, res


SLICE_WIDTHS = (64, 128)  # the column-slice widths nr_pool_score_sliced is built for
SLICE_W = 128             # the width ``sliced=True`` means (the engine's: engine.SLICED_W)


def slice_width(sliced) -> int:
    """``sliced`` of pool_score as a slice width: 0 for today's kernel (False / None / 0),
    SLICE_W for True, else one of SLICE_WIDTHS."""
    if sliced is None or sliced is False or (not isinstance(sliced, bool) and sliced == 0):
        return 0
    w = SLICE_W if sliced is True else int(sliced)
    if w not in SLICE_WIDTHS:
        raise _lib.NewsRecHIPError(f"sliced must be a bool or a slice width of {SLICE_WIDTHS}, got {sliced!r}")
    return w


def slice_table(table: torch.Tensor, slice_w: int, parts: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Slice-major image [1024 / slice_w, N, parts * slice_w] of a row-major [N, parts * 1024]
    table (nr_slice_table): slice s of row r holds columns s * slice_w .. of each part.  A
    bit-exact permutation, into ``out`` when given."""
    dev = _dev(table, out)
    if slice_w not in SLICE_WIDTHS or parts not in (1, 2):
        raise _lib.NewsRecHIPError(f"slice_table: slice_w of {SLICE_WIDTHS}, parts 1 or 2")
    ld = _rowmajor(table, "table")
    n = table.shape[0]
    if table.shape[1] != parts * 1024:
        raise _lib.NewsRecHIPError(f"slice_table: table must be [N, {parts * 1024}]")
    shape = (1024 // slice_w, n, parts * slice_w)
    if out is None:
        out = torch.empty(shape, dtype=table.dtype, device=dev)
    if out.dtype != table.dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.NewsRecHIPError(f"slice_table: out must be contiguous {table.dtype} of shape {shape}")
    if n:
        _lib.call("nr_slice_table", _dtype(table, "table"), n, parts, slice_w, _ptr(table), ld, _ptr(out), 0,
                  _stream(dev))
    return out


def unslice_table(image: torch.Tensor, parts: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row-major [N, parts * 1024] table of a slice_table image (the inverse permutation)."""
    dev = _dev(image, out)
    if image.dim() != 3 or not image.is_contiguous() or parts not in (1, 2) or image.shape[2] % parts:
        raise _lib.NewsRecHIPError("unslice_table: image must be a contiguous [S, N, parts * slice_w] tensor")
    s, n, pw = image.shape
    slice_w = pw // parts
    if slice_w not in SLICE_WIDTHS or s * slice_w != 1024:
        raise _lib.NewsRecHIPError(f"unslice_table: not an image of slice width {SLICE_WIDTHS}")
    if out is None:
        out = torch.empty((n, parts * 1024), dtype=image.dtype, device=dev)
    if out.dtype != image.dtype or tuple(out.shape) != (n, parts * 1024):
        raise _lib.NewsRecHIPError(f"unslice_table: out must be {image.dtype} of shape {(n, parts * 1024)}")
    if n:
        _lib.call("nr_slice_table", _dtype(image, "image"), n, parts, slice_w, _ptr(image), _rowmajor(out, "out"),
                  _ptr(out), 1, _stream(dev))
    return out


def pool_score_sliced_workspace_bytes(slice_w: int, n_imp: int, n_cand: int) -> int:
    """nr_pool_score_sliced_workspace_bytes; raises on arguments the entry refuses."""
    need = int(_lib.load().nr_pool_score_sliced_workspace_bytes(slice_w, n_imp, n_cand))
    if need < 0:
        raise _lib.NewsRecHIPError(_lib.load().nr_last_error().decode() or "nr_pool_score_sliced_workspace_bytes")
    return need


def _check_image(image: torch.Tensor, table: torch.Tensor, slice_w: int, parts: int, name: str) -> None:
    shape = (1024 // slice_w, table.shape[0], parts * slice_w)
    if image.dtype != table.dtype or tuple(image.shape) != shape or not image.is_contiguous():
        raise _lib.NewsRecHIPError(f"{name} must be the contiguous {table.dtype} slice_table image of shape {shape}")


def pool_score(pooler: str, hist_table: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
               hist_idx: torch.Tensor, hist_off: torch.Tensor, cand_idx: torch.Tensor, cand_off: torch.Tensor,
               n_cand: int, want_users: bool = False, scores: Optional[torch.Tensor] = None, sliced=False,
               hist_image: Optional[torch.Tensor] = None, cand_image: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None):
    """Fused history pooling + cosine scoring; returns (scores[C] f32, users[I, D] f32 or None).

    ``n_cand`` = cand_off[-1] (passed by the caller so no device sync is needed).

    ``sliced`` (False: today's kernel; True: slice width SLICE_W; 64 or 128: that width)
    runs nr_pool_score_sliced on the tables' slice images instead, at any size: the same
    scores up to f32 reassociation (the dot is summed per slice), and not the bits that
    recommend, explain and the rest restate -- those are today's kernel's.  ``hist_image`` /
    ``cand_image`` are slice_table images of the two tables a caller keeps (built here when
    absent), ``workspace`` a uint8 buffer of pool_score_sliced_workspace_bytes.  No
    ``want_users`` on this path.
    """
    dev = _dev(hist_table, cand_table, cand_inv_norm, hist_idx, hist_off, cand_idx, cand_off, scores, hist_image,
               cand_image, workspace)
    slice_w = slice_width(sliced)
    if slice_w and want_users:
        raise _lib.NewsRecHIPError("pool_score: the sliced path has no users output (sliced=False)")
    _check_csr(hist_idx, hist_off, "hist")
    _check_csr(cand_idx, cand_off, "cand")
    if hist_off.numel() != cand_off.numel():
        raise _lib.NewsRecHIPError("hist_off and cand_off must both have n_imp + 1 entries")
    if hist_table.dtype != cand_table.dtype:
        raise _lib.NewsRecHIPError("hist_table and cand_table must share a dtype")
    _check_inv_norm(cand_inv_norm, cand_table.shape[0], contiguous=False)
    n_imp = hist_off.numel() - 1
    dim = cand_table.shape[1]
    # empty CSR arrays have no storage; the kernel never reads them (offsets are
    # all equal) but the C-ABI rejects null pointers, so hand it a 1-slot dummy
    one = None
    if hist_idx.numel() == 0 or cand_idx.numel() == 0 or n_cand == 0:
        one = torch.zeros(1, dtype=torch.int32, device=dev)
    if hist_idx.numel() == 0:
        hist_idx = one
    if cand_idx.numel() == 0:
        cand_idx = one
    if scores is None:
        scores = torch.empty(n_cand, dtype=torch.float32, device=dev)
    # zero-element tensors report data_ptr() == 0: give the kernel a real (unread) slot
    scores_buf = scores if scores.numel() > 0 else torch.empty(1, dtype=torch.float32, device=dev)
    if slice_w:
        if n_imp == 0:
            return scores, None
        parts = 2 if pooler == "final" else 1
        if hist_table.dim() != 2 or hist_table.shape[1] != parts * 1024 or tuple(cand_table.shape[1:]) != (1024,):
            raise _lib.NewsRecHIPError(f"pool_score: the sliced path needs a [N, {parts * 1024}] history table and a "
                                       "[N, 1024] candidate table")
        if hist_image is None:
            hist_image = slice_table(hist_table, slice_w, parts)
        if cand_image is None:
            cand_image = slice_table(cand_table, slice_w)
        _check_image(hist_image, hist_table, slice_w, parts, "hist_image")
        _check_image(cand_image, cand_table, slice_w, 1, "cand_image")
        need = max(pool_score_sliced_workspace_bytes(slice_w, n_imp, n_cand), 256)
        ws = grow_workspace(workspace, need, dev)
        _lib.call("nr_pool_score_sliced", POOLERS[pooler], _dtype(cand_table, "cand_table"), dim, slice_w,
                  _ptr(hist_image), hist_table.shape[0], _ptr(cand_image), cand_table.shape[0], _ptr(cand_inv_norm),
                  _ptr(hist_idx), _ptr(hist_off), _ptr(cand_idx), _ptr(cand_off), n_imp, n_cand, _ptr(scores_buf),
                  _ptr(ws), ws.numel(), _stream(dev))
        return scores, None
    users = torch.empty((n_imp, dim), dtype=torch.float32, device=dev) if want_users else None
    _lib.call("nr_pool_score", POOLERS[pooler], _dtype(cand_table, "cand_table"), dim, _ptr(hist_table),
              _rowmajor(hist_table, "hist_table"), _ptr(cand_table), _rowmajor(cand_table, "cand_table"),
              _ptr(cand_inv_norm), _ptr(hist_idx), _ptr(hist_off), _ptr(cand_idx), _ptr(cand_off), n_imp,
              _ptr(scores_buf), _ptr(users) if users is not None and users.numel() else None, _stream(dev))
    return scores, users


def pool_users(pooler: str, hist_table: torch.Tensor, hist_idx: torch.Tensor, hist_off: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pooling only (nr_pool_score with no candidates): users [n, D] f32, one
    row per history segment (into ``out`` when given)."""
    dev = _dev(hist_table, hist_idx, hist_off, out)
    _check_csr(hist_idx, hist_off, "hist")
    n, dim = hist_off.numel() - 1, hist_table.shape[1] if pooler != "final" else hist_table.shape[1] // 2
    if out is not None and (out.dtype != torch.float32 or out.shape != (n, dim) or not out.is_contiguous()):
        raise _lib.NewsRecHIPError(f"pool_users: out must be contiguous f32 {(n, dim)}")
    users = torch.empty((n, dim), dtype=torch.float32, device=dev) if out is None else out
    if n == 0:
        return users
    hidx = hist_idx if hist_idx.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("nr_pool_score", POOLERS[pooler], _dtype(hist_table, "hist_table"), dim, _ptr(hist_table),
              _rowmajor(hist_table, "hist_table"), None, 0, None, _ptr(hidx), _ptr(hist_off), None, None, n, None,
              _ptr(users), _stream(dev))
    return users


def score_users(users: torch.Tensor, user_idx: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
                cand_idx: torch.Tensor, cand_off: torch.Tensor, n_cand: int,
                scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scores of every impression's candidates against users[user_idx[i]]
    (nr_score_users); bit-identical to the fused pool_score pass."""
    dev = _dev(users, user_idx, cand_table, cand_inv_norm, cand_idx, cand_off, scores)
    _check_csr(cand_idx, cand_off, "cand")
    if users.dtype != torch.float32 or not users.is_contiguous() or user_idx.dtype != torch.int32:
        raise _lib.NewsRecHIPError("score_users: users contiguous f32, user_idx int32")
    if user_idx.numel() != cand_off.numel() - 1:
        raise _lib.NewsRecHIPError("score_users: one user index per impression")
    if scores is None:
        scores = torch.empty(n_cand, dtype=torch.float32, device=dev)
    if n_cand == 0 or user_idx.numel() == 0:
        return scores
    _lib.call("nr_score_users", _dtype(cand_table, "cand_table"), cand_table.shape[1], _ptr(users), _ptr(user_idx),
              _ptr(cand_table), _rowmajor(cand_table, "cand_table"), _ptr(cand_inv_norm), _ptr(cand_idx),
              _ptr(cand_off), user_idx.numel(), _ptr(scores), _stream(dev))
    return scores


def topk_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_workspace_bytes (include/newsrec_topk.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_users: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"k in [1, {_lib.NR_TOPK_MAX}], N <= 2^22)")
    return need


def _check_filter(what: str, n_users: int, n_news: int, news_time, time_lo, time_hi, news_cat, cat_mask) -> list:
    """Host checks of a catalogue filter (include/newsrec_filter.h); the five pointers in
    the C order.  The uint64 masks travel as int64 tensors (the same 64 bits)."""
    if (news_time is None) != (time_lo is None) or (news_time is None) != (time_hi is None):
        raise _lib.NewsRecHIPError(f"{what}: news_time, time_lo and time_hi go together")
    if (news_cat is None) != (cat_mask is None):
        raise _lib.NewsRecHIPError(f"{what}: news_cat and cat_mask go together")
    for t, name, dt, n in ((news_time, "news_time", torch.int32, n_news), (time_lo, "time_lo", torch.int32, n_users),
                           (time_hi, "time_hi", torch.int32, n_users), (news_cat, "news_cat", torch.uint8, n_news),
                           (cat_mask, "cat_mask", torch.int64, n_users)):
        if t is not None and (t.dtype != dt or t.dim() != 1 or t.numel() != n or not t.is_contiguous()):
            raise _lib.NewsRecHIPError(f"{what}: {name} must be contiguous {dt} [{n}]")
    return [_ptr(news_time), _ptr(time_lo), _ptr(time_hi), _ptr(news_cat), _ptr(cat_mask)]


def topk_users(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
               excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
               out=None, workspace: Optional[torch.Tensor] = None, _filter=None, _prior=None):
    """The k best rows of ``cand_table`` per user row (nr_topk_users): returns
    (idx int32 [U, k], scores f32 [U, k]), score descending, ties by ascending row,
    a short tail as (-1, -inf); the scores are score_users' bit for bit.  The CSR
    (excl_idx int32, excl_off int64 [U + 1]) lists rows a user must not get; its
    entries are range-checked here (one small sync).  ``out`` = (idx, scores) to
    write into."""
    dev = _dev(users, cand_table, cand_inv_norm, excl_idx, excl_off, workspace, *(out or ()), *(_filter or ()),
               *(_prior or ()))
    n_users, dim, n_news, ld, dt, excl_idx = _check_scan("topk_users", users, cand_table, cand_inv_norm, excl_idx,
                                                         excl_off)
    k = int(k)
    if _prior is not None:  # topk_users_prior: (idx, scores, keys)
        pptr = _check_prior("topk_users_prior", n_users, n_news, *_prior)
        fptr = _check_filter("topk_users_prior", n_users, n_news, *(_filter or (None,) * 5))
        idx, scores, keys = _keyed_outputs("topk_users_prior", out, (n_users, k), dev)
        ws = grow_workspace(workspace, topk_users_prior_workspace_bytes(cand_table.dtype, n_users, n_news, k), dev)
        _lib.call("nr_topk_users_prior", dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld,
                  _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, *pptr, k, _ptr(idx), _ptr(scores),
                  _ptr(keys), _ptr(ws), ws.numel(), _stream(dev))
        return idx, scores, keys
    if out is None:
        idx = torch.empty((n_users, k), dtype=torch.int32, device=dev)
        scores = torch.empty((n_users, k), dtype=torch.float32, device=dev)
    else:
        idx, scores = out
        if (idx.dtype != torch.int32 or scores.dtype != torch.float32 or idx.shape != (n_users, k)
                or scores.shape != (n_users, k) or not idx.is_contiguous() or not scores.is_contiguous()):
            raise _lib.NewsRecHIPError(f"topk_users: out must be contiguous (int32, f32) of shape {(n_users, k)}")
    ws = grow_workspace(workspace, topk_workspace_bytes(cand_table.dtype, n_users, n_news, k), dev)
    fptr = [] if _filter is None else _check_filter("topk_users_filtered", n_users, n_news, *_filter)
    _lib.call("nr_topk_users" if _filter is None else "nr_topk_users_filtered", dt, dim, n_users, _ptr(users), n_news,
              _ptr(cand_table), ld, _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, k, _ptr(idx),
              _ptr(scores), _ptr(ws), ws.numel(), _stream(dev))
    return idx, scores


def topk_users_filtered(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                        news_time: Optional[torch.Tensor] = None, time_lo: Optional[torch.Tensor] = None,
                        time_hi: Optional[torch.Tensor] = None, news_cat: Optional[torch.Tensor] = None,
                        cat_mask: Optional[torch.Tensor] = None, excl_idx: Optional[torch.Tensor] = None,
                        excl_off: Optional[torch.Tensor] = None, out=None, workspace: Optional[torch.Tensor] = None):
    """topk_users under a catalogue filter (nr_topk_users_filtered): row c is eligible for
    user u when it is not excluded, ``time_lo[u] <= news_time[c] <= time_hi[u]`` (int32 [N],
    int32 [U]; both bounds inclusive, lo > hi is an empty window) and bit ``news_cat[c]``
    (uint8 [N]; 64 or more is never eligible) of ``cat_mask[u]`` (int64 [U], read as
    uint64) is set.  Either pair may be left out; with neither the result is topk_users'
    bit for bit.  Everything else is topk_users' contract with "eligible" so defined."""
    return topk_users(users, cand_table, cand_inv_norm, k, excl_idx=excl_idx, excl_off=excl_off, out=out,
                      workspace=workspace, _filter=(news_time, time_lo, time_hi, news_cat, cat_mask))


def _check_prior(what: str, n_users: int, n_news: int, news_prior, user_gain) -> list:
    """Host checks of a rank-one prior (include/newsrec_prior.h): the two pointers in the C
    order.  Both or neither; f32 [N] and f32 [U].  (Finite values are the caller's promise,
    as for the table: PoolScoreEngine checks what it is given on the host.)"""
    if (news_prior is None) != (user_gain is None):
        raise _lib.NewsRecHIPError(f"{what}: news_prior and user_gain go together")
    for t, name, n in ((news_prior, "news_prior", n_news), (user_gain, "user_gain", n_users)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous()):
            raise _lib.NewsRecHIPError(f"{what}: {name} must be contiguous {torch.float32} [{n}]")
    return [_ptr(news_prior), _ptr(user_gain)]


def _keyed_outputs(what: str, out, shape, dev):
    """(idx int32, scores f32, keys f32) of ``shape``: the caller's ``out`` checked, or new ones."""
    if out is None:
        return (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                torch.empty(shape, dtype=torch.float32, device=dev))
    if len(out) != 3 or any(t is None or t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                            for t, dt in zip(out, (torch.int32, torch.float32, torch.float32))):
        raise _lib.NewsRecHIPError(f"{what}: out must be contiguous (int32, f32, f32) of shape {tuple(shape)}")
    return tuple(out)


def topk_users_prior_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_users_prior_workspace_bytes (include/newsrec_prior.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_users_prior_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_users_prior: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"k in [1, {_lib.NR_TOPK_MAX}], N <= 2^22)")
    return need


def topk_users_prior(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                     news_prior: Optional[torch.Tensor] = None, user_gain: Optional[torch.Tensor] = None,
                     news_time: Optional[torch.Tensor] = None, time_lo: Optional[torch.Tensor] = None,
                     time_hi: Optional[torch.Tensor] = None, news_cat: Optional[torch.Tensor] = None,
                     cat_mask: Optional[torch.Tensor] = None, excl_idx: Optional[torch.Tensor] = None,
                     excl_off: Optional[torch.Tensor] = None, out=None, workspace: Optional[torch.Tensor] = None):
    """topk_users_filtered with a rank-one prior (nr_topk_users_prior): news are selected and
    ordered by ``cosine + user_gain[u] * news_prior[c]`` (f32 [N], f32 [U]).  Returns (idx
    int32 [U, k], scores f32 [U, k], keys f32 [U, k]): the scores are still score_users' bit
    for bit, ``keys = fl32(scores + fl32(gain * prior))`` is what the list is ordered by
    (descending, ties by ascending row; a short tail is (-1, -inf, -inf)).  A user with gain
    0 gets topk_users_filtered's list; a zero user is ordered by the prior alone.  Without
    the pair the result is topk_users_filtered's bit for bit and keys == scores.  ``out`` =
    (idx, scores, keys) to write into."""
    return topk_users(users, cand_table, cand_inv_norm, k, excl_idx=excl_idx, excl_off=excl_off, out=out,
                      workspace=workspace, _filter=(news_time, time_lo, time_hi, news_cat, cat_mask),
                      _prior=(news_prior, user_gain))


def topk_users_after_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_users_after_workspace_bytes (include/newsrec_page.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_users_after_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_users_after: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"k in [1, {_lib.NR_TOPK_MAX}], N <= 2^22)")
    return need


def start_cursor(n: int, device):
    """The cursor in front of the first row of ``n`` users' lists: (key f32 [n] = +inf,
    row int32 [n] = -1).  topk_users_after from it is topk_users_after without a cursor."""
    return (torch.full((n,), float("inf"), dtype=torch.float32, device=device),
            torch.full((n,), -1, dtype=torch.int32, device=device))


def _check_cursor(what: str, name: str, n_users: int, cursor) -> list:
    """A cursor pair (key f32 [U], row int32 [U]) as the two pointers of the C call."""
    if cursor is None:
        return [None, None]
    if (not isinstance(cursor, (tuple, list)) or len(cursor) != 2
            or any(not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or t.numel() != n_users
                   or not t.is_contiguous() for t, dt in zip(cursor, (torch.float32, torch.int32)))):
        raise _lib.NewsRecHIPError(f"{what}: {name} must be (key contiguous {torch.float32} [{n_users}], "
                                   f"row contiguous {torch.int32} [{n_users}])")
    return [_ptr(cursor[0]), _ptr(cursor[1])]


def topk_users_after(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                     after=None, want_next: bool = True, excl_idx: Optional[torch.Tensor] = None,
                     excl_off: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                     time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                     news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                     news_prior: Optional[torch.Tensor] = None, user_gain: Optional[torch.Tensor] = None, out=None,
                     workspace: Optional[torch.Tensor] = None, next_out=None, excl_checked: bool = False,
                     _what: str = "topk_users_after"):
    """topk_users_prior behind a cursor (nr_topk_users_after): the k best eligible rows that lie
    strictly after ``after`` = (key f32 [U], row int32 [U]) in the order the retrieval selects in
    (selection key descending, row ascending).  Returns (idx, scores, keys, next): the first
    three as topk_users_prior returns them (keys == scores without a prior), ``next`` the cursor
    behind the call's last row -- feed it back for the next k rows -- or the end cursor
    (-inf, INT32_MAX) where fewer than k rows were left; None without ``want_next``.  Pages
    are consecutive, disjoint slices of one ordering; inside a page the order is by score (by
    key under a prior).  A cursor is opaque: selection keys, valid only with the same user
    row, table, dtype, prior and gain; exclusion lists and filters may change between pages.
    ``after`` = None (or start_cursor) starts the list.  ``out`` = (idx, scores, keys) and
    ``next_out`` = (key, row) to write into; ``next_out`` may be ``after`` itself.
    ``excl_checked`` promises that an earlier call range-checked these exclusion lists, and
    saves their sync: a walk over several pages then never waits for the device."""
    what = _what  # (topk_users_deep runs this body against its own entry and workspace)
    dev = _dev(users, cand_table, cand_inv_norm, news_prior, user_gain, news_time, time_lo, time_hi, news_cat,
               cat_mask, excl_idx, excl_off, workspace, *(out or ()), *(after or ()), *(next_out or ()))
    n_users, dim, n_news, ld, dt, excl_idx = _check_scan(what, users, cand_table, cand_inv_norm, excl_idx, excl_off,
                                                         check_rows=not excl_checked)
    k = int(k)
    pptr = _check_prior(what, n_users, n_news, news_prior, user_gain)
    fptr = _check_filter(what, n_users, n_news, news_time, time_lo, time_hi, news_cat, cat_mask)
    aptr = _check_cursor(what, "after", n_users, after)
    nxt = next_out
    if nxt is None and want_next:
        nxt = (torch.empty(n_users, dtype=torch.float32, device=dev), torch.empty(n_users, dtype=torch.int32, device=dev))
    nptr = _check_cursor(what, "next_out", n_users, nxt)
    ws_bytes = {"topk_users_deep": topk_users_deep_workspace_bytes,
                "topk_request": topk_request_workspace_bytes}.get(what, topk_users_after_workspace_bytes)
    ws = grow_workspace(workspace, ws_bytes(cand_table.dtype, n_users, n_news, k), dev)
    idx, scores, keys = _keyed_outputs(what, out, (n_users, k), dev)
    _lib.call("nr_" + what, dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld,
              _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, *pptr, *aptr, *nptr, k, _ptr(idx),
              _ptr(scores), _ptr(keys), _ptr(ws), ws.numel(), _stream(dev))
    return idx, scores, keys, (None if nxt is None else tuple(nxt))


def topk_users_deep_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_users_deep_workspace_bytes (include/newsrec_deep.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_users_deep_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_users_deep: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"k in [1, {_lib.NR_TOPK_DEEP_MAX}], N <= 2^22)")
    return need


def topk_users_deep(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                    after=None, want_next: bool = True, excl_idx: Optional[torch.Tensor] = None,
                    excl_off: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                    time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                    news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                    news_prior: Optional[torch.Tensor] = None, user_gain: Optional[torch.Tensor] = None, out=None,
                    workspace: Optional[torch.Tensor] = None, next_out=None, excl_checked: bool = False):
    """topk_users_after for k up to 256 from ONE walk over the table (nr_topk_users_deep): the
    arguments and the result (idx, scores, keys, next) are topk_users_after's.  The rows are
    exactly those of the ceil(k / 64) cursor pages topk_users_after would return from ``after``
    (the last page asking for the remainder), ordered as one list by score (by key under a
    prior), ties by ascending row; ``next`` is the cursor behind the last of those pages, so
    deep calls chain like pages do.  The table is multiplied once instead of once per page; the
    workspace holds 4 KiB per user and run of chunks (topk_users_deep_workspace_bytes).  For
    k <= 64 it is topk_users_after bit for bit."""
    return topk_users_after(users, cand_table, cand_inv_norm, k, after=after, want_next=want_next, excl_idx=excl_idx,
                            excl_off=excl_off, news_time=news_time, time_lo=time_lo, time_hi=time_hi,
                            news_cat=news_cat, cat_mask=cat_mask, news_prior=news_prior, user_gain=user_gain, out=out,
                            workspace=workspace, next_out=next_out, excl_checked=excl_checked,
                            _what="topk_users_deep")


def topk_request_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_request_workspace_bytes (include/newsrec_request.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_request_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_request: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"U in [1, {_lib.NR_REQUEST_MAX_USERS}] (topk_users_after takes more users), "
            f"k in [1, {_lib.NR_TOPK_MAX}], N <= 2^22)")
    return need


def topk_request(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                 after=None, want_next: bool = True, excl_idx: Optional[torch.Tensor] = None,
                 excl_off: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                 time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                 news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                 news_prior: Optional[torch.Tensor] = None, user_gain: Optional[torch.Tensor] = None, out=None,
                 workspace: Optional[torch.Tensor] = None, next_out=None, excl_checked: bool = False):
    """topk_users_after for at most 32 users at the cost of one read of the table
    (nr_topk_request): the arguments and the result (idx, scores, keys, next) are
    topk_users_after's, bit for bit, and a cursor of either continues in the other.  One
    workgroup per run of nr_topk_request_run_rows(N) table rows keeps the user rows in LDS and
    streams the table past them, where topk_users_after's 128-user tiles would be padding.
    ``out``, ``next_out`` and ``workspace`` (topk_request_workspace_bytes) let a caller hold
    every buffer across calls.  More than 32 users: use topk_users_after."""
    if users.dim() == 2 and users.shape[0] > _lib.NR_REQUEST_MAX_USERS:
        raise _lib.NewsRecHIPError(f"topk_request: {users.shape[0]} users (at most {_lib.NR_REQUEST_MAX_USERS}; "
                                   "topk_users_after takes more)")
    return topk_users_after(users, cand_table, cand_inv_norm, k, after=after, want_next=want_next, excl_idx=excl_idx,
                            excl_off=excl_off, news_time=news_time, time_lo=time_lo, time_hi=time_hi,
                            news_cat=news_cat, cat_mask=cat_mask, news_prior=news_prior, user_gain=user_gain, out=out,
                            workspace=workspace, next_out=next_out, excl_checked=excl_checked, _what="topk_request")


def topk_users_capped_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, k: int) -> int:
    """nr_topk_users_capped_workspace_bytes (include/newsrec_caps.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_users_capped_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_users_capped: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, k = {k}; "
            f"k in [1, {_lib.NR_TOPK_MAX}], N <= 2^22)")
    return need


def _check_groups(what: str, n_news: int, news_group, cap) -> int:
    """Host checks of per-group caps (include/newsrec_caps.h): ``news_group`` 16-bit integers
    [N] (int16, or uint16 where torch has it: the same bits) with every label in [0,
    NR_CAP_GROUPS_MAX) -- read back here, one small sync -- and ``cap`` in [1, NR_TOPK_MAX]."""
    ok16 = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
    if (not isinstance(news_group, torch.Tensor) or news_group.dtype not in ok16 or news_group.dim() != 1
            or news_group.numel() != n_news or not news_group.is_contiguous()):
        raise _lib.NewsRecHIPError(f"{what}: news_group must be contiguous 16-bit integers [{n_news}]")
    if isinstance(cap, bool) or int(cap) != cap or not 1 <= int(cap) <= _lib.NR_TOPK_MAX:
        raise _lib.NewsRecHIPError(f"{what}: cap = {cap!r} outside [1, {_lib.NR_TOPK_MAX}]")
    if n_news:
        lo, hi = (int(v) for v in torch.aminmax(news_group.view(torch.int16)))
        if lo < 0 or hi >= _lib.NR_CAP_GROUPS_MAX:
            raise _lib.NewsRecHIPError(f"{what}: news_group labels must lie in [0, {_lib.NR_CAP_GROUPS_MAX})")
    return int(cap)


def topk_users_capped(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int,
                      news_group: torch.Tensor, cap: int, news_prior: Optional[torch.Tensor] = None,
                      user_gain: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                      time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                      news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                      excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None, out=None,
                      workspace: Optional[torch.Tensor] = None):
    """topk_users_prior with at most ``cap`` rows of one group per list (nr_topk_users_capped):
    ``news_group`` [N] 16-bit labels in [0, 1024) (data_utils.dense_groups makes them), ``cap``
    in [1, 64].  The list is the greedy one: eligible rows in the order (key descending, row
    ascending), a row taken while its group holds fewer than ``cap``, until k are taken; it is
    short, ending in (-1, -inf, -inf), when the caps leave fewer than k rows.  Returns (idx,
    scores, keys) as topk_users_prior does; without a prior keys == scores.  ``cap >= k`` is
    topk_users_prior bit for bit.  The filter, the prior and the exclusion CSR compose."""
    what = "topk_users_capped"
    dev = _dev(users, cand_table, cand_inv_norm, news_group, news_prior, user_gain, news_time, time_lo, time_hi,
               news_cat, cat_mask, excl_idx, excl_off, workspace, *(out or ()))
    n_users, dim, n_news, ld, dt, excl_idx = _check_scan(what, users, cand_table, cand_inv_norm, excl_idx, excl_off)
    k = int(k)
    cap = _check_groups(what, n_news, news_group, cap)
    pptr = _check_prior(what, n_users, n_news, news_prior, user_gain)
    fptr = _check_filter(what, n_users, n_news, news_time, time_lo, time_hi, news_cat, cat_mask)
    ws = grow_workspace(workspace, topk_users_capped_workspace_bytes(cand_table.dtype, n_users, n_news, k), dev)
    idx, scores, keys = _keyed_outputs(what, out, (n_users, k), dev)
    _lib.call("nr_topk_users_capped", dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld,
              _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, *pptr, _ptr(news_group), cap, k, _ptr(idx),
              _ptr(scores), _ptr(keys), _ptr(ws), ws.numel(), _stream(dev))
    return idx, scores, keys


def section_masks(sections) -> list:
    """``sections`` (a sequence of 64-bit masks: Python ints, int64 or uint64) as a list of
    Python ints in [0, 2^64): the same 64 bits whichever way they came."""
    if isinstance(sections, torch.Tensor):
        sections = sections.reshape(-1).tolist()
    return [int(v) & 0xFFFFFFFFFFFFFFFF for v in sections]


def topk_sections_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, n_sections: int, k: int) -> int:
    """nr_topk_sections_workspace_bytes (include/newsrec_sections.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_sections_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, n_sections, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_sections: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, S = {n_sections}, "
            f"k = {k}; S in [1, {_lib.NR_SECTIONS_MAX}], k >= 1, S * k <= {_lib.NR_TOPK_MAX}, N <= 2^22)")
    return need


def topk_sections(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int, sections,
                  news_cat: torch.Tensor, news_time: Optional[torch.Tensor] = None,
                  time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                  excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None, out=None,
                  workspace: Optional[torch.Tensor] = None, _prior=None):
    """The k best eligible rows of each of S sections per user row, from one walk over the
    table (nr_topk_sections): returns (idx int32 [U, S, k], scores f32 [U, S, k]).
    ``sections`` is a sequence of S disjoint 64-bit category masks (Python ints, int64 or
    uint64), the same for every user; ``news_cat`` uint8 [N].  Section s of the result
    equals topk_users_filtered(k, cat_mask = sections[s]) with the same time window and
    exclusion lists, bit for bit."""
    dev = _dev(users, cand_table, cand_inv_norm, news_cat, news_time, time_lo, time_hi, excl_idx, excl_off, workspace,
               *(out or ()), *(_prior or ()))
    n_users, dim, n_news, ld, dt, excl_idx = _check_scan("topk_sections", users, cand_table, cand_inv_norm, excl_idx,
                                                         excl_off)
    if (news_cat is None or news_cat.dtype != torch.uint8 or news_cat.dim() != 1 or news_cat.numel() != n_news
            or not news_cat.is_contiguous()):
        raise _lib.NewsRecHIPError(f"topk_sections: news_cat must be contiguous torch.uint8 [{n_news}]")
    masks = section_masks(sections)
    n_sec, k = len(masks), int(k)
    tptr = _check_filter("topk_sections", n_users, n_news, news_time, time_lo, time_hi, None, None)[:3]
    tptr.append(_ptr(news_cat))
    shape = (n_users, n_sec, k)
    sec = (ctypes.c_uint64 * n_sec)(*masks)  # read on the host, before the call returns
    if _prior is not None:  # topk_sections_prior: (idx, scores, keys)
        pptr = _check_prior("topk_sections_prior", n_users, n_news, *_prior)
        need = topk_sections_prior_workspace_bytes(cand_table.dtype, n_users, n_news, n_sec, k)
        idx, scores, keys = _keyed_outputs("topk_sections_prior", out, shape, dev)
        ws = grow_workspace(workspace, need, dev)
        _lib.call("nr_topk_sections_prior", dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld,
                  _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *tptr, ctypes.cast(sec, ctypes.c_void_p), *pptr,
                  n_sec, k, _ptr(idx), _ptr(scores), _ptr(keys), _ptr(ws), ws.numel(), _stream(dev))
        return idx, scores, keys
    need = topk_sections_workspace_bytes(cand_table.dtype, n_users, n_news, n_sec, k)
    if out is None:
        idx = torch.empty(shape, dtype=torch.int32, device=dev)
        scores = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        idx, scores = out
        if (idx.dtype != torch.int32 or scores.dtype != torch.float32 or tuple(idx.shape) != shape
                or tuple(scores.shape) != shape or not idx.is_contiguous() or not scores.is_contiguous()):
            raise _lib.NewsRecHIPError(f"topk_sections: out must be contiguous (int32, f32) of shape {shape}")
    ws = grow_workspace(workspace, need, dev)
    _lib.call("nr_topk_sections", dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld, _ptr(cand_inv_norm),
              _ptr(excl_idx), _ptr(excl_off), *tptr, ctypes.cast(sec, ctypes.c_void_p), n_sec, k, _ptr(idx),
              _ptr(scores), _ptr(ws), ws.numel(), _stream(dev))
    return idx, scores


def topk_sections_prior_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, n_sections: int, k: int) -> int:
    """nr_topk_sections_prior_workspace_bytes (include/newsrec_prior.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_topk_sections_prior_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, n_sections, k))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"topk_sections_prior: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, S = {n_sections}, "
            f"k = {k}; S in [1, {_lib.NR_SECTIONS_MAX}], k >= 1, S * k <= {_lib.NR_TOPK_MAX}, N <= 2^22)")
    return need


def topk_sections_prior(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, k: int, sections,
                        news_cat: torch.Tensor, news_prior: Optional[torch.Tensor] = None,
                        user_gain: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                        time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                        excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None, out=None,
                        workspace: Optional[torch.Tensor] = None):
    """topk_sections with topk_users_prior's rank-one prior (nr_topk_sections_prior): returns
    (idx int32 [U, S, k], scores f32 [U, S, k], keys f32 [U, S, k]).  Section s equals
    topk_users_prior(k, cat_mask = sections[s]) with the same prior, time window and
    exclusion lists, bit for bit, keys included."""
    return topk_sections(users, cand_table, cand_inv_norm, k, sections, news_cat, news_time=news_time,
                         time_lo=time_lo, time_hi=time_hi, excl_idx=excl_idx, excl_off=excl_off, out=out,
                         workspace=workspace, _prior=(news_prior, user_gain))


def rank_targets_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, n_targets: int) -> int:
    """nr_rank_targets_workspace_bytes (include/newsrec_fullrank.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_rank_targets_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, n_targets))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"rank_targets: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, T = {n_targets}; "
            "U >= 1, 1 <= N <= 2^22, T < 2^31)")
    return need


def rank_targets(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, tgt_idx: torch.Tensor,
                 tgt_off: torch.Tensor, excl_idx: Optional[torch.Tensor] = None,
                 excl_off: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None, _filter=None, _prior=None) -> torch.Tensor:
    """Full-table ranks of target rows (nr_rank_targets): for the targets
    tgt_idx[tgt_off[u]:tgt_off[u + 1]] (int32, int64 [U + 1]) of user row u, int32 [T]
    with the number of eligible rows of ``cand_table`` that beat the target in top-K's
    order (score descending, ties by ascending row); 0 is the best row, -1 a target
    that is excluded itself or outside the table.  For k <= 64 the targets with
    rank < k are exactly the rows topk_users returns.  The exclusion CSR is as
    topk_users takes it; its entries and the target offsets are checked here (one
    small sync).  ``out`` = int32 [T] to write into."""
    dev = _dev(users, cand_table, cand_inv_norm, tgt_idx, tgt_off, excl_idx, excl_off, workspace, out,
               *(_filter or ()), *(_prior or ()))
    n_users, dim, n_news, ld, dt, excl_idx = _check_scan("rank_targets", users, cand_table, cand_inv_norm, excl_idx,
                                                         excl_off)
    _check_csr(tgt_idx, tgt_off, "tgt")
    n_tgt = tgt_idx.numel()
    if tgt_off.numel() != n_users + 1:
        raise _lib.NewsRecHIPError("rank_targets: tgt_off must have U + 1 entries")
    if (int(tgt_off[0]) != 0 or int(tgt_off[-1]) != n_tgt
            or (n_users > 1 and not bool((tgt_off[1:] >= tgt_off[:-1]).all()))):
        raise _lib.NewsRecHIPError(f"rank_targets: tgt_off must ascend from 0 to the {n_tgt} targets")
    if out is None:
        out = torch.empty(n_tgt, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.shape != (n_tgt,) or not out.is_contiguous():
        raise _lib.NewsRecHIPError(f"rank_targets: out must be contiguous int32 of shape {(n_tgt,)}")
    if _prior is not None:  # rank_targets_prior
        pptr = _check_prior("rank_targets_prior", n_users, n_news, *_prior)
        fptr = _check_filter("rank_targets_prior", n_users, n_news, *(_filter or (None,) * 5))
        ws = grow_workspace(workspace, rank_targets_prior_workspace_bytes(cand_table.dtype, n_users, n_news, n_tgt),
                            dev)
        if n_tgt:
            _lib.call("nr_rank_targets_prior", dt, dim, n_users, _ptr(users), n_news, _ptr(cand_table), ld,
                      _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, *pptr, n_tgt, _ptr(tgt_idx),
                      _ptr(tgt_off), _ptr(out), _ptr(ws), ws.numel(), _stream(dev))
        return out
    ws = grow_workspace(workspace, max(rank_targets_workspace_bytes(cand_table.dtype, n_users, n_news, n_tgt), 256), dev)
    fptr = [] if _filter is None else _check_filter("rank_targets_filtered", n_users, n_news, *_filter)
    if n_tgt == 0:
        return out
    _lib.call("nr_rank_targets" if _filter is None else "nr_rank_targets_filtered", dt, dim, n_users, _ptr(users),
              n_news, _ptr(cand_table), ld, _ptr(cand_inv_norm), _ptr(excl_idx), _ptr(excl_off), *fptr, n_tgt,
              _ptr(tgt_idx), _ptr(tgt_off), _ptr(out), _ptr(ws), ws.numel(), _stream(dev))
    return out


def rank_targets_filtered(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
                          tgt_idx: torch.Tensor, tgt_off: torch.Tensor, news_time: Optional[torch.Tensor] = None,
                          time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                          news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                          excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rank_targets under topk_users_filtered's catalogue filter (nr_rank_targets_filtered):
    only eligible rows are counted, and a target that is itself ineligible -- excluded,
    outside its user's window or of an unwanted category -- gets -1.  For k <= 64 the
    targets with rank < k are exactly the rows topk_users_filtered returns."""
    return rank_targets(users, cand_table, cand_inv_norm, tgt_idx, tgt_off, excl_idx=excl_idx, excl_off=excl_off,
                        out=out, workspace=workspace, _filter=(news_time, time_lo, time_hi, news_cat, cat_mask))


def rank_targets_prior_workspace_bytes(dtype: torch.dtype, n_users: int, n_news: int, n_targets: int) -> int:
    """nr_rank_targets_prior_workspace_bytes (include/newsrec_prior.h); raises on a shape the entry refuses."""
    need = int(_lib.load().nr_rank_targets_prior_workspace_bytes(_DT.get(dtype, -1), n_users, n_news, n_targets))
    if need < 0:
        raise _lib.NewsRecHIPError(
            f"rank_targets_prior: unsupported shape (dtype {dtype}, U = {n_users}, N = {n_news}, T = {n_targets}; "
            "U >= 1, 1 <= N <= 2^22, T < 2^31)")
    return need


def rank_targets_prior(users: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
                       tgt_idx: torch.Tensor, tgt_off: torch.Tensor, news_prior: Optional[torch.Tensor] = None,
                       user_gain: Optional[torch.Tensor] = None, news_time: Optional[torch.Tensor] = None,
                       time_lo: Optional[torch.Tensor] = None, time_hi: Optional[torch.Tensor] = None,
                       news_cat: Optional[torch.Tensor] = None, cat_mask: Optional[torch.Tensor] = None,
                       excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rank_targets_filtered under topk_users_prior's rank-one prior (nr_rank_targets_prior): the
    eligible rows are counted on the keys ``cosine + user_gain[u] * news_prior[c]``.  For
    k <= 64 the targets with rank < k are exactly the rows topk_users_prior returns."""
    return rank_targets(users, cand_table, cand_inv_norm, tgt_idx, tgt_off, excl_idx=excl_idx, excl_off=excl_off,
                        out=out, workspace=workspace, _filter=(news_time, time_lo, time_hi, news_cat, cat_mask),
                        _prior=(news_prior, user_gain))


def rerank_mmr(cand_table: torch.Tensor, cand_inv_norm: torch.Tensor, list_idx: torch.Tensor, list_rel: torch.Tensor,
               k: int, lam: float, want_pos: bool = False, want_ild: bool = False, want_sim: bool = False, out=None):
    """Greedy MMR re-ranking of retrieved lists (nr_rerank_mmr, include/newsrec_rerank.h):
    ``list_idx`` int32 [U, M] rows of ``cand_table`` with relevance ``list_rel`` f32 [U, M]
    (e.g. topk_users' result, M <= 64; an index outside the table is a pad).  k of the M are
    picked one at a time, each maximising lam * rel - (1 - lam) * (largest cosine to an
    entry already picked); ties go to the lower position.  Returns (idx int32 [U, k],
    rel f32 [U, k]) in pick order, a short tail as (-1, -inf), followed by those asked
    for of: pos int32 [U, k] (positions in the input list), ild f32 [U, 2] (intra-list
    diversity of the input's first k valid entries and of the picks), sim f32 [U, M, M]
    (the cosine matrix, diagonal and pads 0).  ``out`` = (idx, rel, pos, ild, sim) to
    write into, None for the ones not wanted."""
    dev = _dev(cand_table, cand_inv_norm, list_idx, list_rel, *(out or ()))
    ld = _rowmajor(cand_table, "cand_table")
    n_news, dim = cand_table.shape
    dt = _dtype(cand_table, "cand_table")
    _check_inv_norm(cand_inv_norm, n_news)
    if list_idx.dtype != torch.int32 or list_idx.dim() != 2 or not list_idx.is_contiguous():
        raise _lib.NewsRecHIPError("rerank_mmr: list_idx must be contiguous int32 [U, M]")
    if list_rel.dtype != torch.float32 or list_rel.shape != list_idx.shape or not list_rel.is_contiguous():
        raise _lib.NewsRecHIPError("rerank_mmr: list_rel must be contiguous f32 of list_idx's shape")
    n_users, m = list_idx.shape
    k, lam = int(k), float(lam)
    if not 1 <= m <= _lib.NR_RERANK_MAX or not 1 <= k <= m:
        raise _lib.NewsRecHIPError(f"rerank_mmr: need 1 <= k <= M <= {_lib.NR_RERANK_MAX}, got k = {k}, M = {m}")
    if not 0.0 <= lam <= 1.0:  # NaN fails too
        raise _lib.NewsRecHIPError(f"rerank_mmr: lam = {lam} outside [0, 1]")
    spec = (("idx", torch.int32, (n_users, k), True), ("rel", torch.float32, (n_users, k), True),
            ("pos", torch.int32, (n_users, k), want_pos), ("ild", torch.float32, (n_users, 2), want_ild),
            ("sim", torch.float32, (n_users, m, m), want_sim))
    out, res = _outputs("rerank_mmr", spec, out, dev)
    if n_users == 0:
        return res
    _lib.call("nr_rerank_mmr", dt, dim, n_users, n_news, _ptr(cand_table), ld, _ptr(cand_inv_norm), _ptr(list_idx),
              _ptr(list_rel), m, k, lam, *(_ptr(t) for t in out), _stream(dev))
    return res


def explain_scores(pooler: str, hist_table: torch.Tensor, cand_table: torch.Tensor, cand_inv_norm: torch.Tensor,
                   hist_idx: torch.Tensor, hist_off: torch.Tensor, list_idx: torch.Tensor, top: int = 3,
                   want_sum: bool = False, want_matrix: bool = False, out=None):
    """Exact per-click attribution of scores (nr_explain_scores, include/newsrec_explain.h):
    for user u with history hist_idx[hist_off[u]:hist_off[u + 1]] (rows of ``hist_table``,
    pool_score's layout) and the listed rows ``list_idx`` int32 [U, K] of ``cand_table``
    (K <= 64; an index outside the table is a pad), the additive contribution of every
    click to every listed news' score.  Returns (top_pos int32 [U, K, top], top_val f32
    [U, K, top]) -- the history positions of the ``top`` <= 8 largest contributions, value
    descending, ties by ascending position, a short tail as (-1, -inf) -- followed by
    those asked for of: sums f32 [U, K] (the contributions' sums: pool_score's scores),
    matrix f32 [len(hist_idx), K] (every contribution, row = CSR row of the click).
    ``top`` = 0 leaves the top lists out.  ``out`` = (top_pos, top_val, sums, matrix) to
    write into, None for the ones not wanted."""
    dev = _dev(hist_table, cand_table, cand_inv_norm, hist_idx, hist_off, list_idx, *(out or ()))
    if pooler not in POOLERS:
        raise _lib.NewsRecHIPError(f"explain_scores: unknown pooler {pooler!r}")
    _check_csr(hist_idx, hist_off, "hist")
    hld, ld = _rowmajor(hist_table, "hist_table"), _rowmajor(cand_table, "cand_table")
    n_news, dim = cand_table.shape
    dt = _dtype(cand_table, "cand_table")
    if hist_table.dtype != cand_table.dtype:
        raise _lib.NewsRecHIPError("hist_table and cand_table must share a dtype")
    if hist_table.shape[1] != (2 * dim if pooler == "final" else dim):
        raise _lib.NewsRecHIPError(f"explain_scores: hist_table rows must be {'2 x ' if pooler == 'final' else ''}"
                                   f"{dim} wide for the {pooler} pooler")
    _check_inv_norm(cand_inv_norm, n_news)
    if list_idx.dtype != torch.int32 or list_idx.dim() != 2 or not list_idx.is_contiguous():
        raise _lib.NewsRecHIPError("explain_scores: list_idx must be contiguous int32 [U, K]")
    n_users, k = list_idx.shape
    if hist_off.numel() != n_users + 1:
        raise _lib.NewsRecHIPError("explain_scores: hist_off must have U + 1 entries")
    top = int(top)
    if not 1 <= k <= _lib.NR_TOPK_MAX:
        raise _lib.NewsRecHIPError(f"explain_scores: need 1 <= K <= {_lib.NR_TOPK_MAX}, got K = {k}")
    if not 0 <= top <= _lib.NR_EXPLAIN_TOP_MAX:
        raise _lib.NewsRecHIPError(f"explain_scores: top = {top} outside [0, {_lib.NR_EXPLAIN_TOP_MAX}]")
    if not (top or want_sum or want_matrix):
        raise _lib.NewsRecHIPError("explain_scores: nothing requested (top = 0, no sums, no matrix)")
    n_hist = hist_idx.numel()
    spec = (("top_pos", torch.int32, (n_users, k, top), top > 0), ("top_val", torch.float32, (n_users, k, top), top > 0),
            ("sums", torch.float32, (n_users, k), want_sum), ("matrix", torch.float32, (n_hist, k), want_matrix))
    bufs, res = _outputs("explain_scores", spec, out, dev, real_slots=True)
    if n_users == 0:
        return res
    if want_matrix and int(hist_off[-1]) != n_hist:  # the matrix has one row per CSR row (one small sync)
        raise _lib.NewsRecHIPError(f"explain_scores: hist_off ends at {int(hist_off[-1])}, hist_idx has {n_hist} rows")
    hidx = hist_idx if n_hist else torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("nr_explain_scores", POOLERS[pooler], dt, dim, _ptr(hist_table), hld, n_news, _ptr(cand_table), ld,
              _ptr(cand_inv_norm), n_users, _ptr(hidx), _ptr(hist_off), _ptr(list_idx), k, max(top, 1),
              *(_ptr(t) for t in bufs), _stream(dev))
    return res


def dense_rank(scores: torch.Tensor, cand_off: torch.Tensor, check: bool = True) -> torch.Tensor:
    """Per-impression dense descending ranks (int32), scipy rankdata(-x, 'dense')."""
    dev = _dev(scores, cand_off)
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise _lib.NewsRecHIPError("dense_rank: scores must be contiguous f32")
    ranks = torch.empty(scores.numel(), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("nr_dense_rank", _ptr(scores), _ptr(cand_off), cand_off.numel() - 1, _ptr(ranks), _ptr(status),
              _stream(dev))
    if check and int(status.item()) != 0:
        raise _lib.NewsRecHIPError("dense_rank: an impression has more than 2048 candidates")
    return ranks


def impression_metrics(ranks: torch.Tensor, labels: torch.Tensor, cand_off: torch.Tensor):
    """Per-impression (AUC, MRR, nDCG@5, nDCG@10) f64 [n, 4] + tie flags int32 [n]
    from dense ranks (int32) and 0/1 labels (f32); raises on >2048 candidates or
    non-binary labels."""
    dev = _dev(ranks, labels, cand_off)
    if ranks.dtype != torch.int32 or labels.dtype != torch.float32 or cand_off.dtype != torch.int64:
        raise _lib.NewsRecHIPError("impression_metrics: ranks int32, labels f32, cand_off int64")
    n = cand_off.numel() - 1
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    tie = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("nr_impression_metrics", _ptr(ranks), _ptr(labels), _ptr(cand_off), n, _ptr(out), _ptr(tie),
              _ptr(status), _stream(dev))
    st = int(status.item())
    if st & 1:
        raise _lib.NewsRecHIPError("impression_metrics: an impression has more than 2048 candidates")
    if st & 2:
        raise _lib.NewsRecHIPError("impression_metrics: labels must be 0/1 and ranks in 1..c")
    return out, tie


def final_attn_transform(emb: torch.Tensor, w: dict, out: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-news FinalAttention table [n, 2*1024] = (x, exp(w)) in emb.dtype.

    ``w`` holds device weights in emb.dtype (W1..W5) and f32 biases (b1..b4).
    """
    dev = _dev(emb, out)
    dt = _dtype(emb, "emb")
    n, dim = emb.shape
    if dim != 1024:
        raise _lib.NewsRecHIPError("final_attn_transform: dim must be 1024")
    if out is None:
        out = torch.empty((n, 2 * dim), dtype=emb.dtype, device=dev)
    need = _lib.load().nr_final_attn_workspace_bytes(dt, n)
    workspace = grow_workspace(workspace, need, dev)
    for k in ("W1", "W2", "W3", "W4", "W5"):
        if w[k].dtype != emb.dtype or not w[k].is_contiguous():
            raise _lib.NewsRecHIPError(f"final_attn_transform: {k} must be contiguous {emb.dtype}")
    _lib.call("nr_final_attn_transform", dt, n, _ptr(emb), _rowmajor(emb, "emb"), _ptr(w["W1"]), _ptr(w["b1"]),
              _ptr(w["W2"]), _ptr(w["b2"]), _ptr(w["W3"]), _ptr(w["b3"]), _ptr(w["W4"]), _ptr(w["b4"]),
              _ptr(w["W5"]), _ptr(out), _ptr(workspace), need, _stream(dev))
    return out


def latent_transform(emb: torch.Tensor, w: dict, out: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-news LatentAttention table [n, 1024] (the pre-pooling hiddens)."""
    dev = _dev(emb, out)
    dt = _dtype(emb, "emb")
    n, dim = emb.shape
    if dim != 1024:
        raise _lib.NewsRecHIPError("latent_transform: dim must be 1024")
    if out is None:
        out = torch.empty((n, dim), dtype=emb.dtype, device=dev)
    need = _lib.load().nr_latent_workspace_bytes(dt, n)
    workspace = grow_workspace(workspace, need, dev)
    for k in ("A", "Bt", "W1i", "W2"):
        if w[k].dtype != emb.dtype or not w[k].is_contiguous():
            raise _lib.NewsRecHIPError(f"latent_transform: {k} must be contiguous {emb.dtype}")
    if dt == _lib.NR_BF16 and "Wq_ln" in w:
        # both LayerNorms folded into the GEMMs that consume them (latent_attention.lnfold_weights)
        _lib.call("nr_latent_transform_lnfold", dt, n, _ptr(emb), _rowmajor(emb, "emb"), _ptr(w["Wq_ln"]),
                  _ptr(w["ucq"]), _ptr(w["Bt"]), _ptr(w["Wf_ln"]), _ptr(w["ucf"]), _ptr(w["W2"]), _ptr(w["b2"]),
                  _ptr(out), _ptr(workspace), need, _stream(dev))
        return out
    _lib.call("nr_latent_transform", dt, n, _ptr(emb), _rowmajor(emb, "emb"), _ptr(w["lnq_g"]), _ptr(w["lnq_b"]),
              _ptr(w["A"]), _ptr(w["Bt"]), _ptr(w["lnf_g"]), _ptr(w["lnf_b"]), _ptr(w["W1i"]), _ptr(w["b1i"]),
              _ptr(w["W2"]), _ptr(w["b2"]), _ptr(out), _ptr(workspace), need, _stream(dev))
    return out


def embed_ln(ids: torch.Tensor, pos: torch.Tensor, word: torch.Tensor, pos_emb: torch.Tensor, type_emb: torch.Tensor,
             gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LN(word[ids] + type_emb + pos_emb[pos]) for packed token rows (XLM-R embeddings)."""
    dev = _dev(ids, pos, word, pos_emb, type_emb, gamma, beta, out)
    if ids.dtype != torch.int32 or pos.dtype != torch.int32:
        raise _lib.NewsRecHIPError("embed_ln: ids/pos must be int32")
    if word.shape[1] != 1024:
        raise _lib.NewsRecHIPError("embed_ln: hidden size must be 1024")
    n = ids.numel()
    if out is None:
        out = torch.empty((n, 1024), dtype=word.dtype, device=dev)
    _lib.call("nr_embed_ln", _dtype(word, "word"), n, _ptr(ids), _ptr(pos), _ptr(word), _ptr(pos_emb),
              _ptr(type_emb), _ptr(gamma), _ptr(beta), ctypes.c_float(eps), _ptr(out), _stream(dev))
    return out


def attention_varlen(qkv: torch.Tensor, cu_seqlens: torch.Tensor, qblock_off: torch.Tensor, n_qblocks: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-head x 64 self-attention per packed sequence: qkv [T, 3072] -> ctx [T, 1024]."""
    dev = _dev(qkv, cu_seqlens, qblock_off, out)
    if qkv.shape[1] != 3072 or not qkv.is_contiguous():
        raise _lib.NewsRecHIPError("attention_varlen: qkv must be contiguous [T, 3072]")
    if cu_seqlens.dtype != torch.int32 or qblock_off.dtype != torch.int32:
        raise _lib.NewsRecHIPError("attention_varlen: offsets must be int32")
    if out is None:
        out = torch.empty((qkv.shape[0], 1024), dtype=qkv.dtype, device=dev)
    _lib.call("nr_attention_varlen", _dtype(qkv, "qkv"), cu_seqlens.numel() - 1, n_qblocks, _ptr(qkv),
              _ptr(cu_seqlens), _ptr(qblock_off), _ptr(out), _stream(dev))
    return out


def pool_rows(pooler: str, table: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    """Pool consecutive rows per segment (segment i = rows off[i]..off[i+1]-1):
    users [n_seg, 1024] f32 ("mean" = average_pool, "latent" = + F.normalize,
    "final" = FinalAttention pooling of [x | exp(w)] rows)."""
    dev = _dev(table, off)
    if off.dtype != torch.int64 or not off.is_contiguous():
        raise _lib.NewsRecHIPError("pool_rows: off must be contiguous int64")
    n_seg = off.numel() - 1
    users = torch.empty((n_seg, 1024), dtype=torch.float32, device=dev)
    if n_seg == 0:
        return users
    _lib.call("nr_pool_score", POOLERS[pooler], _dtype(table, "table"), 1024, _ptr(table), _rowmajor(table, "table"),
              None, 0, None, None, _ptr(off), None, None, n_seg, None, _ptr(users), _stream(dev))
    return users


_ENC_POOL = {"mean": _lib.NR_POOL_MEAN, "normalize": _lib.NR_POOL_LATENT, None: _lib.NR_POOL_NONE}


def encoder_forward(layers, emb: dict, ids: torch.Tensor, seq_lens: torch.Tensor, n_tokens: int,
                    pool: Optional[str] = "mean", want_hidden: bool = False, eps: float = 1e-5,
                    workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """Whole XLM-R forward through ``nr_encoder_forward`` (one C-ABI call).

    layers: a ctypes array of ``_lib.EncoderLayer``; emb: word / pos / type
    embedding tensors (dtype of the weights) and LN gamma / beta (f32); ids
    int32 [n_tokens] and seq_lens int32 [n_seq] on the device.  Returns
    (pooled [n_seq, 1024] f32 or None, hidden [n_tokens, 1024] or None)."""
    dev = _dev(ids, seq_lens, emb["word"], workspace, status)
    if ids.dtype != torch.int32 or seq_lens.dtype != torch.int32 or not ids.is_contiguous():
        raise _lib.NewsRecHIPError("encoder_forward: ids / seq_lens must be contiguous int32")
    dt = _dtype(emb["word"], "word")
    n_seq = seq_lens.numel()
    pooled = torch.empty((n_seq, 1024), dtype=torch.float32, device=dev) if pool else None
    hidden = torch.empty((n_tokens, 1024), dtype=emb["word"].dtype, device=dev) if want_hidden else None
    need = _lib.load().nr_encoder_workspace_bytes(dt, n_tokens, n_seq)
    workspace = grow_workspace(workspace, need, dev)
    _lib.call("nr_encoder_forward", dt, len(layers), ctypes.cast(layers, ctypes.c_void_p) if len(layers) else None,
              _ptr(emb["word"]), emb["word"].shape[0], _ptr(emb["pos"]), emb["pos"].shape[0], _ptr(emb["type"]),
              _ptr(emb["ln_g"]), _ptr(emb["ln_b"]), ctypes.c_float(eps), n_seq, n_tokens, _ptr(seq_lens), _ptr(ids),
              _ENC_POOL[pool], _ptr(pooled), _ptr(hidden), _ptr(status), _ptr(workspace), need, _stream(dev))
    return pooled, hidden


# ------------------------------------------------------------------ training step (config 5)
def _grouped_arrays(problems, mnk):
    """The (M, N, K, A, lda, W, ldw, C, ldc) ctypes arrays of grouped (a, w, out)
    problems whose sizes are ``mnk`` = [(M, N, K), ...]."""
    n = len(problems)
    L, P = ctypes.c_int64 * n, ctypes.c_void_p * n
    M, N, K = (L(*d) for d in zip(*mnk))
    a, w, out = zip(*problems)
    ptrs = lambda ts: P(*[t.data_ptr() for t in ts])
    lds = lambda ts, name: L(*[_rowmajor(t, name) for t in ts])
    return M, N, K, ptrs(a), lds(a, "a"), ptrs(w), lds(w, "w"), ptrs(out), lds(out, "out")


def gemm_grouped(problems) -> None:
    """out_i = a_i @ w_i.T for up to 8 (a, w, out) triples in ONE launch over all
    their 256x256 tiles (nr_gemm_grouped): small GEMMs that cannot fill the
    chip alone run side by side.  bf16 or f32 a/w, f32 or bf16 out (one out dtype)."""
    problems = list(problems)
    if not 1 <= len(problems) <= 8:
        raise _lib.NewsRecHIPError("gemm_grouped: 1..8 problems")
    dev = _dev(*[t for pr in problems for t in pr])
    for i, (a, w, out) in enumerate(problems):
        if a.dtype != w.dtype or a.shape[1] != w.shape[1] or tuple(out.shape) != (a.shape[0], w.shape[0]):
            raise _lib.NewsRecHIPError(f"gemm_grouped: problem {i} shape/dtype mismatch")
        if out.dtype != problems[0][2].dtype:
            raise _lib.NewsRecHIPError("gemm_grouped: all outputs must share a dtype")
    arrays = _grouped_arrays(problems, [(a.shape[0], w.shape[0], a.shape[1]) for a, w, _ in problems])
    _lib.call("nr_gemm_grouped", _dtype(problems[0][0], "a"), _dtype(problems[0][2], "out"), len(problems), *arrays,
              _stream(dev))


def gemm_grouped_tn(problems, alpha=None) -> None:
    """out_i = alpha_i * a_i.T @ w_i for up to 8 (a, w, out) triples in ONE launch
    (nr_gemm_grouped_tn): a_i [K, M], w_i [K, N] bf16 row-major (the weight grads
    dOut^T X straight from the activations), out_i [M, N] f32 or bf16."""
    problems = list(problems)
    if not 1 <= len(problems) <= 8:
        raise _lib.NewsRecHIPError("gemm_grouped_tn: 1..8 problems")
    dev = _dev(*[t for pr in problems for t in pr])
    n = len(problems)
    al = (ctypes.c_float * n)(*([1.0] * n if alpha is None else alpha))
    for i, (a, w, out) in enumerate(problems):
        if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or a.shape[0] != w.shape[0] \
                or tuple(out.shape) != (a.shape[1], w.shape[1]):
            raise _lib.NewsRecHIPError(f"gemm_grouped_tn: problem {i} shape/dtype mismatch")
        if out.dtype != problems[0][2].dtype:
            raise _lib.NewsRecHIPError("gemm_grouped_tn: all outputs must share a dtype")
    arrays = _grouped_arrays(problems, [(a.shape[1], w.shape[1], a.shape[0]) for a, w, _ in problems])
    _lib.call("nr_gemm_grouped_tn", _dtype(problems[0][2], "out"), n, *arrays, al, _stream(dev))


def gemm_relu_dropout(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], seed: int, p: float,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = relu(a @ w.T + bias) * keep / (1 - p), keep from the (seed, row, col) hash stream."""
    dev = _dev(a, w, bias, out)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=dev)
    _lib.call("nr_gemm_relu_dropout", _dtype(a, "a"), _dtype(out, "out"), M, N, K, _ptr(a), _rowmajor(a, "a"), _ptr(w),
              _rowmajor(w, "w"), _ptr(bias), _ptr(out), _rowmajor(out, "out"), ctypes.c_uint64(seed & (2**64 - 1)),
              ctypes.c_float(p), _stream(dev))
    return out


def gemm_drelu(a: torch.Tensor, w: torch.Tensor, y: torch.Tensor, scale: float,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (y > 0) ? (a @ w.T) * scale : 0 (backward of relu + dropout, y = forward output)."""
    dev = _dev(a, w, y, out)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=y.dtype, device=dev)
    _lib.call("nr_gemm_drelu", _dtype(a, "a"), _dtype(out, "out"), M, N, K, _ptr(a), _rowmajor(a, "a"), _ptr(w),
              _rowmajor(w, "w"), _ptr(y), _rowmajor(y, "y"), _ptr(out), _rowmajor(out, "out"), ctypes.c_float(scale),
              _stream(dev))
    return out


def splitk_fixup(partials: torch.Tensor, out: torch.Tensor, epilogue: str = "none", bias: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, row0: int = 0, seed: int = 0, p: float = 0.0,
                 scale: float = 1.0) -> torch.Tensor:
    """out = epi(partials.sum(0) + bias) for K-slice partials [parts, rows, N] f32
    (nr_splitk_fixup): epilogue "none", "relu_dropout" (mask rows row0..), "drelu"
    (residual = the forward output), "resadd" (+ residual) or "exp"."""
    dev = _dev(partials, out, bias, residual)
    epi = {"none": _lib.NR_EPI_NONE, "relu_dropout": _lib.NR_EPI_RELU_DROPOUT, "drelu": _lib.NR_EPI_DRELU,
           "resadd": _lib.NR_EPI_RESADD, "exp": _lib.NR_EPI_EXP}[epilogue]
    if partials.dtype != torch.float32 or not partials.is_contiguous() or partials.dim() != 3:
        raise _lib.NewsRecHIPError("splitk_fixup: partials must be contiguous f32 [parts, rows, N]")
    parts, rows, N = partials.shape
    if tuple(out.shape) != (rows, N):
        raise _lib.NewsRecHIPError("splitk_fixup: out must be [rows, N]")
    _lib.call("nr_splitk_fixup", _dtype(out, "out"), epi, rows, N, parts, _ptr(partials), _ptr(bias), _ptr(residual),
              _rowmajor(residual, "residual") if residual is not None else 0, _ptr(out), _rowmajor(out, "out"), row0,
              ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_float(p), ctypes.c_float(scale), _stream(dev))
    return out


def gather_rows(src: torch.Tensor, idx: Optional[torch.Tensor], n: Optional[int] = None,
                out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = _dev(src, idx, out)
    n = idx.numel() if idx is not None else (n if n is not None else src.shape[0])
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous()):
        raise _lib.NewsRecHIPError("gather_rows: idx must be contiguous int32")
    dim = src.shape[1]
    if out is None:
        out = torch.empty((n, dim), dtype=out_dtype or src.dtype, device=dev)
    _lib.call("nr_gather_rows", _dtype(src, "src"), _dtype(out, "out"), n, dim, _ptr(src), _rowmajor(src, "src"),
              _ptr(idx), _ptr(out), _rowmajor(out, "out"), _stream(dev))
    return out


def transpose(src: torch.Tensor, out_dtype: Optional[torch.dtype] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dev = _dev(src, out)
    rows, cols = src.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=out_dtype or src.dtype, device=dev)
    _lib.call("nr_transpose", _dtype(src, "src"), _dtype(out, "out"), rows, cols, _ptr(src), _rowmajor(src, "src"),
              _ptr(out), _rowmajor(out, "out"), _stream(dev))
    return out


def final_pool_fwd(xp: torch.Tensor, off: torch.Tensor):
    dev = _dev(xp, off)
    n_seg = off.numel() - 1
    users = torch.empty((n_seg, 1024), dtype=torch.float32, device=dev)
    z = torch.empty_like(users)
    _lib.call("nr_final_pool_fwd", _dtype(xp, "xp"), n_seg, _ptr(off), _ptr(xp), _rowmajor(xp, "xp"), _ptr(users),
              _ptr(z), _stream(dev))
    return users, z


def final_pool_bwd(xp: torch.Tensor, off: torch.Tensor, users: torch.Tensor, z: torch.Tensor, du: torch.Tensor,
                   dx: torch.Tensor, dw: torch.Tensor) -> None:
    dev = _dev(xp, off, users, z, du, dx, dw)
    _lib.call("nr_final_pool_bwd", _dtype(xp, "xp"), off.numel() - 1, _ptr(off), dx.shape[0], _ptr(xp),
              _rowmajor(xp, "xp"), _ptr(users), _ptr(z), _ptr(du), _ptr(dx), _rowmajor(dx, "dx"), _ptr(dw),
              _rowmajor(dw, "dw"), _stream(dev))


def cosine_margin(users: torch.Tensor, E: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, margin: float,
                  loss: torch.Tensor, du: torch.Tensor, dE: torch.Tensor,
                  s_out: Optional[torch.Tensor] = None) -> None:
    dev = _dev(users, E, pos, neg, loss, du, dE, s_out)
    _lib.call("nr_cosine_margin", users.shape[0], _ptr(users), _ptr(E), _rowmajor(E, "E"), _ptr(pos), _ptr(neg),
              ctypes.c_float(margin), _ptr(s_out), _ptr(loss), _ptr(du), _ptr(dE), _stream(dev))


def _check_contrastive(cand, target, mask, B: int):
    """dtype / shape checks of the InfoNCE stage's index tensors; returns Cn."""
    if cand.dtype != torch.int32 or target.dtype != torch.int32 or not cand.is_contiguous() or not target.is_contiguous():
        raise _lib.NewsRecHIPError("cand and target must be contiguous int32")
    Cn = cand.numel()
    if target.numel() != B:
        raise _lib.NewsRecHIPError(f"target must have one column per batch row ({target.numel()} != {B})")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_contiguous() or tuple(mask.shape) != (B, Cn)):
        raise _lib.NewsRecHIPError(f"mask must be a contiguous uint8 [{B}, {Cn}] tensor")
    return Cn


def cosine_infonce(users: torch.Tensor, E: torch.Tensor, cand: torch.Tensor, target: torch.Tensor,
                   mask: Optional[torch.Tensor] = None, temperature: float = 1.0, want_logits: bool = False):
    """InfoNCE over in-batch candidate columns (nr_cosine_infonce, the sibling of
    ``cosine_margin``; trainer.py:612-625): users [B, 1024] f32, E [U, >= 1024] f32,
    cand [Cn] int32 (-1 = pad), target [B] int32, mask None or uint8 [B, Cn] (1 =
    left out).  Returns (loss [1], du [B, 1024], dE_cols [Cn, 1024] -- per column,
    not scattered -- and the logits [B, Cn] with -inf where excluded, or None)."""
    dev = _dev(users, E, cand, target, mask)
    if users.dtype != torch.float32 or E.dtype != torch.float32 or not users.is_contiguous() or users.shape[1] != 1024:
        raise _lib.NewsRecHIPError("users must be contiguous float32 [B, 1024] and E float32")
    B = users.shape[0]
    Cn = _check_contrastive(cand, target, mask, B)
    need = int(_lib.load().nr_cosine_infonce_workspace_bytes(B, Cn))
    if need < 0:
        raise _lib.NewsRecHIPError(f"nr_cosine_infonce: bad shape B = {B}, Cn = {Cn}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    du = torch.empty((B, 1024), dtype=torch.float32, device=dev)
    dE = torch.empty((Cn, 1024), dtype=torch.float32, device=dev)
    logits = torch.empty((B, Cn), dtype=torch.float32, device=dev) if want_logits else None
    _lib.call("nr_cosine_infonce", B, Cn, _ptr(users), _ptr(E), _rowmajor(E, "E"), _ptr(cand), _ptr(target), _ptr(mask),
              ctypes.c_float(1.0 / temperature), _ptr(logits), _ptr(loss), _ptr(du), _ptr(dE), _ptr(ws), ws.numel(),
              _stream(dev))
    return loss, du, dE, logits


def scatter_add_rows(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor) -> None:
    dev = _dev(src, idx, dst)
    _lib.call("nr_scatter_add_rows", _dtype(src, "src"), idx.numel(), src.shape[1], _ptr(src), _rowmajor(src, "src"),
              _ptr(idx), _ptr(dst), _rowmajor(dst, "dst"), _stream(dev))


def col_sum(src: torch.Tensor, out: torch.Tensor) -> None:
    dev = _dev(src, out)
    _lib.call("nr_col_sum", _dtype(src, "src"), src.shape[0], src.shape[1], _ptr(src), _rowmajor(src, "src"), _ptr(out),
              _stream(dev))


def ln_param_grad(x: torch.Tensor, row_idx: Optional[torch.Tensor], eps: float, dy: torch.Tensor,
                  dgamma: torch.Tensor, dbeta: torch.Tensor) -> None:
    dev = _dev(x, row_idx, dy, dgamma, dbeta)
    dt = TOKEN_DT[x.dtype]
    n = row_idx.numel() if row_idx is not None else x.shape[0]
    _lib.call("nr_ln_param_grad", dt, n, x.shape[1], _ptr(x), _rowmajor(x, "x"), _ptr(row_idx), ctypes.c_float(eps),
              _ptr(dy), _rowmajor(dy, "dy"), _ptr(dgamma), _ptr(dbeta), _stream(dev))


def sumsq(x: torch.Tensor, out: torch.Tensor) -> None:
    dev = _dev(x, out)
    _lib.call("nr_sumsq", x.numel(), _ptr(x), _ptr(out), _stream(dev))


def adamw(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float,
          betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, max_norm: float = 0.0,
          sumsq_t: Optional[torch.Tensor] = None, p_bf16: Optional[torch.Tensor] = None) -> None:
    dev = _dev(p, g, m, v, sumsq_t, p_bf16)
    _lib.call("nr_adamw", p.numel(), _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), step, ctypes.c_float(lr),
              ctypes.c_float(betas[0]), ctypes.c_float(betas[1]), ctypes.c_float(eps), ctypes.c_float(weight_decay),
              ctypes.c_float(max_norm), _ptr(sumsq_t), _stream(dev))


def _f32(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.float32:
        raise _lib.NewsRecHIPError(f"{name}: the latent-attention training kernels take f32 (got {t.dtype})")


def layernorm_bwd(x: torch.Tensor, gamma: Optional[torch.Tensor], dy: torch.Tensor, eps: float = 1e-5,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of LayerNorm(x; gamma) for upstream dy (+ residual grad), f32."""
    for t, n in ((x, "x"), (dy, "dy")):
        _f32(t, n)
    out = torch.empty_like(x) if out is None else out
    dev = _dev(x, gamma, dy, residual, out)
    _lib.call("nr_layernorm_bwd", x.shape[0], x.shape[1], _ptr(x), _rowmajor(x, "x"), _ptr(gamma),
              ctypes.c_float(eps), _ptr(dy), _rowmajor(dy, "dy"), _ptr(residual),
              _rowmajor(residual, "residual") if residual is not None else 0, _ptr(out), _rowmajor(out, "out"),
              _stream(dev))
    return out


def softmax64_bwd(p: torch.Tensor, dp: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """dS of a softmax over groups of 64 columns, from its output p and upstream dp
    (f32 inputs; dS f32 or bf16)."""
    _f32(p, "p")
    _f32(dp, "dp")
    out = torch.empty(p.shape, dtype=out_dtype, device=p.device)
    dev = _dev(p, dp, out)
    _lib.call("nr_softmax64_bwd", _dtype(out, "out"), p.shape[0], p.shape[1], _ptr(p), _rowmajor(p, "p"), _ptr(dp),
              _rowmajor(dp, "dp"), _ptr(out), _rowmajor(out, "out"), _stream(dev))
    return out


def geglu_fwd(g: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """a * gelu(gates) with a, gates = g.chunk(2, -1) (f32 in, exact erf; out f32 or bf16)."""
    _f32(g, "g")
    f = g.shape[1] // 2
    z = torch.empty((g.shape[0], f), dtype=out_dtype, device=g.device)
    dev = _dev(g, z)
    _lib.call("nr_geglu_fwd", _dtype(z, "z"), g.shape[0], f, _ptr(g), _rowmajor(g, "g"), _ptr(z), f, _stream(dev))
    return z


def geglu_bwd(g: torch.Tensor, dz: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    _f32(g, "g")
    _f32(dz, "dz")
    f = g.shape[1] // 2
    dg = torch.empty(g.shape, dtype=out_dtype, device=g.device)
    dev = _dev(g, dz, dg)
    _lib.call("nr_geglu_bwd", _dtype(dg, "dg"), g.shape[0], f, _ptr(g), _rowmajor(g, "g"), _ptr(dz), _rowmajor(dz, "dz"),
              _ptr(dg), _rowmajor(dg, "dg"), _stream(dev))
    return dg
