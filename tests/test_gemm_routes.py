"""Host routing of nr_gemm (csrc/gemm.hip): every (kernel, dtype pair, epilogue)
a call can reach, at the smallest shapes that reach it, against float64 matmuls
of the same operands (needs an MI355X).

Routes (gemm_dispatch_ex): the 128x128 register-staged kernel takes N % 256 != 0
and outputs / residuals that are not 16-byte aligned; the 256x256 LDS-DMA kernel
takes the rest, except bf16 -> bf16 with an even number of 64-deep K steps, which
runs on the persistent kernel.  M = 300 is ragged for both tile heights (two M
tiles at 256, three at 128); at N = 256 it is two persistent tiles, which at the
default workgroup count run as the half-tile tail.

Tolerances are those of test_gpu_parity.py for the same kernels: f32 in and
out 1e-5, bf16 in / f32 out 1e-4, bf16 out 1e-2 (rtol = atol).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from news_recommendation_project_v2_amd import _lib, ops
from news_recommendation_project_v2_amd.latent_attention import interleave_geglu_rows

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
M = 300
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
NR_ERR_INVALID, NR_ERR_UNSUPPORTED = -1, -3
DRELU_SCALE = 1.25


def _name(dt):
    return "f32" if dt == F32 else "bf16"


def _tol(dt_in, dt_out):
    if dt_out == BF16:
        return 1e-2
    return 1e-5 if dt_in == F32 else 1e-4


# (route, dt_in, dt_out, epilogue, N, K, layout); layout: "plain", "out_off" (output a
# column-offset view off 16-byte alignment) or "res_off" (aligned output, misaligned residual)
def _cases():
    out = []
    for di, do in PAIRS:
        for epi in ("none", "relu", "exp", "gelu", "resadd", "geglu", "drelu", "relu_dropout0"):
            out.append(("t128", di, do, epi, 128, 128, "plain"))
        for epi in ("none", "resadd"):
            out.append(("t128", di, do, epi, 256, 128, "out_off"))
        out.append(("t128", di, do, "resadd", 256, 128, "res_off"))
    for di, do in PAIRS:
        K = 192 if (di, do) == (BF16, BF16) else 128  # an odd K-step count: refused by the persistent kernel
        for epi in ("none", "relu", "exp", "gelu", "resadd", "geglu", "softmax64", "drelu"):
            out.append(("t256", di, do, epi, 256, K, "plain"))
    for epi in ("none", "relu", "exp", "gelu", "resadd", "geglu", "softmax64", "drelu", "softmax64_bwd"):
        out.append(("persistent", BF16, BF16, epi, 256, 128, "plain"))
    return out


CASES = _cases()


def case_id(c):
    route, di, do, epi, N, K, layout = c
    return f"{route}-{_name(di)}-{_name(do)}-{epi}-N{N}-K{K}-{layout}"


@functools.lru_cache(maxsize=None)
def _operands(dt_in, N, K):
    """CPU operands of one (dtype, N, K), shared by every case that uses them (read-only)."""
    g = torch.Generator().manual_seed(1000 * N + K + (7 if dt_in == BF16 else 0))
    a = (torch.randn(M, K, generator=g) * 0.2).to(dt_in)
    w = (torch.randn(N, K, generator=g) * 0.1).to(dt_in)
    b = torch.randn(N, generator=g) * 0.1
    prod = a.double() @ w.double().T
    r = torch.randn(M, N, generator=g)                                      # residual / forward output
    p = torch.softmax(torch.randn(M, N // 64, 64, generator=g), -1).reshape(M, N).bfloat16()
    return {"a": a, "w": w, "b": b, "prod": prod, "acc": prod + b.double(), "r": r, "p": p}


def _reference(c):
    route, di, do, epi, N, K, layout = c
    o = _operands(di, N, K)
    acc = o["acc"]
    if epi in ("relu", "relu_dropout0"):
        return acc.clamp_min(0)
    if epi == "exp":
        return acc.exp()
    if epi == "gelu":
        return torch.nn.functional.gelu(acc)
    if epi == "resadd":
        return acc + o["r"].to(do).double()
    if epi == "geglu":
        return acc[:, :N // 2] * torch.nn.functional.gelu(acc[:, N // 2:])
    if epi == "softmax64":
        return torch.softmax(acc.reshape(M, N // 64, 64), -1).reshape(M, N)
    if epi == "drelu":
        return torch.where(o["r"].to(do).double() > 0, o["prod"] * DRELU_SCALE, torch.zeros_like(acc))
    if epi == "softmax64_bwd":
        p3 = o["p"].double().reshape(M, N // 64, 64)
        d3 = acc.reshape(M, N // 64, 64)
        return (p3 * (d3 - (p3 * d3).sum(-1, keepdim=True))).reshape(M, N)
    return acc


def _offset_view(rows, cols, dt, dev):
    """[rows, cols] view one element into a wider buffer: data pointer 2 or 4 bytes off 16."""
    v = torch.zeros(rows, cols + 8, dtype=dt, device=dev)[:, 1:1 + cols]
    assert v.data_ptr() % 16 != 0
    return v


def launch(c, dev):
    """One launch of case c; returns the output tensor (a view for the offset layouts)."""
    route, di, do, epi, N, K, layout = c
    o = _operands(di, N, K)
    a, w, b = o["a"].to(dev), o["w"], o["b"]
    if epi == "geglu":
        w, b = interleave_geglu_rows(w).contiguous(), interleave_geglu_rows(b).contiguous()
    w, b = w.to(dev), b.to(dev)
    ncols = N // 2 if epi == "geglu" else N
    out = _offset_view(M, ncols, do, dev) if layout == "out_off" else torch.empty(M, ncols, dtype=do, device=dev)
    res = None
    if epi in ("resadd", "drelu", "softmax64_bwd"):
        src = o["p"] if epi == "softmax64_bwd" else o["r"].to(do)
        if layout == "res_off":
            res = _offset_view(M, N, do, dev)
            res.copy_(src)
        else:
            res = src.to(dev)
    if epi == "drelu":
        ops.gemm_drelu(a, w, res, DRELU_SCALE, out=out)
    elif epi == "relu_dropout0":
        ops.gemm_relu_dropout(a, w, b, seed=5, p=0.0, out=out)
    else:
        ops.gemm(a, w, b, epilogue=epi, residual=res, out=out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_route_matches_float64(gpu_device, c):
    route, di, do, epi, N, K, layout = c
    out = launch(c, gpu_device)
    tol = _tol(di, do)
    np.testing.assert_allclose(out.float().cpu().double().numpy(), _reference(c).numpy(), rtol=tol, atol=tol)
    if epi == "relu_dropout0":  # p = 0 keeps everything at scale 1: the relu epilogue's values
        relu = launch((route, di, do, "relu", N, K, layout), gpu_device)
        assert torch.equal(out, relu)


def _raw_gemm(dev, dt_in, dt_out, epi, N, K, with_res=False, out_off=False):
    """nr_gemm through ctypes: (return code, nr_last_error text)."""
    lib = _lib.load()
    code = {F32: _lib.NR_F32, BF16: _lib.NR_BF16}
    a = torch.zeros(M, K, dtype=dt_in, device=dev)
    w = torch.zeros(N, K, dtype=dt_in, device=dev)
    out = _offset_view(M, N, dt_out, dev) if out_off else torch.zeros(M, N, dtype=dt_out, device=dev)
    res = torch.zeros(M, N, dtype=dt_out, device=dev) if with_res else None
    P = ctypes.c_void_p
    rc = lib.nr_gemm(code[dt_in], code[dt_out], epi, M, N, K, P(a.data_ptr()), a.stride(0), P(w.data_ptr()),
                     w.stride(0), None, P(res.data_ptr()) if with_res else None, N if with_res else 0,
                     P(out.data_ptr()), out.stride(0), P(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.nr_last_error().decode(errors="replace")


REFUSALS = [
    ("softmax64_n128", (BF16, BF16, _lib.NR_EPI_SOFTMAX64, 128, 128), NR_ERR_UNSUPPORTED),
    ("softmax64_out_off", (BF16, BF16, _lib.NR_EPI_SOFTMAX64, 256, 128, False, True), NR_ERR_UNSUPPORTED),
    ("softmax64_bwd_f32", (F32, F32, _lib.NR_EPI_SOFTMAX64_BWD, 256, 128, True), NR_ERR_UNSUPPORTED),
    ("softmax64_bwd_k192", (BF16, BF16, _lib.NR_EPI_SOFTMAX64_BWD, 256, 192, True), NR_ERR_UNSUPPORTED),
    ("epilogue_10", (BF16, BF16, 10, 256, 128), NR_ERR_INVALID),
    ("resadd_null_residual", (BF16, BF16, _lib.NR_EPI_RESADD, 256, 128), NR_ERR_INVALID),
    ("n64", (BF16, BF16, _lib.NR_EPI_NONE, 64, 128), NR_ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("name,args,want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(gpu_device, name, args, want):
    rc, msg = _raw_gemm(gpu_device, *args)
    assert rc == want, (name, rc, msg)
    assert msg, name


def test_dropout_stream_is_route_independent(gpu_device):
    """One (M, N, seed) drops the same elements on the persistent kernel, the
    256x256 tile kernel (bf16 -> f32) and the 128x128 kernel (misaligned output):
    with a bias that makes every pre-activation positive, the zeros are the mask."""
    N, K, seed, p = 256, 128, 1234, 0.25
    o = _operands(BF16, N, K)
    a, w = o["a"].to(gpu_device), o["w"].to(gpu_device)
    b = torch.full((N,), 4.0, device=gpu_device)
    assert float(o["prod"].min()) > -3.0
    outs = {
        "persistent": torch.empty(M, N, dtype=BF16, device=gpu_device),
        "t256": torch.empty(M, N, dtype=F32, device=gpu_device),
        "t128": _offset_view(M, N, BF16, gpu_device),
    }
    for out in outs.values():
        ops.gemm_relu_dropout(a, w, b, seed=seed, p=p, out=out)
    torch.cuda.synchronize()
    masks = {k: (v == 0) for k, v in outs.items()}
    frac = float(masks["persistent"].float().mean())
    assert 0.2 < frac < 0.3, frac
    assert torch.equal(masks["persistent"], masks["t256"])
    assert torch.equal(masks["persistent"], masks["t128"])
    keep = ~masks["persistent"]
    ref = ((o["prod"] + 4.0) / (1.0 - p)).to(gpu_device)
    np.testing.assert_allclose(outs["t256"][keep].double().cpu().numpy(), ref[keep].cpu().numpy(), rtol=1e-4, atol=1e-4)
