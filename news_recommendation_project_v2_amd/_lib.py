"""ctypes binding of ``libnewsrec_hip.so`` (C-ABI declared in include/newsrec.h).

The library is built in-tree by ``__graft_entry__.build()`` (or
``make -C news_recommendation_project_v2_amd/csrc``).  There is no CPU or
PyTorch fallback: if the library is missing or a call fails, a
``NewsRecHIPError`` is raised.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
from pathlib import Path
from typing import Optional, Sequence

LIB_PATH = Path(__file__).resolve().with_name("libnewsrec_hip.so")
CSRC = Path(__file__).resolve().with_name("csrc")
INCLUDE = Path(__file__).resolve().parent.parent / "include"
# translation units of libnewsrec_hip.so, in link order (also the hash order)
HIP_SOURCES = ("capi.hip", "gemm.hip", "pool_score.hip", "rowops.hip", "rank.hip", "encoder.hip", "train.hip",
               "metrics.hip", "comm.hip", "latent_train.hip", "final_train.hip", "contrastive.hip", "topk.hip",
               "fullrank.hip", "rerank.hip", "explain.hip", "sections.hip", "caps.hip", "deep.hip",
               "request.hip")
# the headers they include (every object is rebuilt when one changes), hashed after the sources
HIP_HEADERS = (CSRC / "nr_common.h", CSRC / "nr_rows.h", CSRC / "nr_train.h", CSRC / "nr_score_tile.h",
               INCLUDE / "newsrec.h", INCLUDE / "newsrec_contrastive.h", INCLUDE / "newsrec_topk.h",
               INCLUDE / "newsrec_fullrank.h", INCLUDE / "newsrec_rerank.h", INCLUDE / "newsrec_explain.h",
               INCLUDE / "newsrec_filter.h", INCLUDE / "newsrec_sections.h", INCLUDE / "newsrec_prior.h",
               INCLUDE / "newsrec_caps.h", INCLUDE / "newsrec_page.h", INCLUDE / "newsrec_sliced.h", INCLUDE / "newsrec_deep.h",
               INCLUDE / "newsrec_request.h")


def hip_source_files() -> list:
    return [CSRC / s for s in HIP_SOURCES] + list(HIP_HEADERS)


def source_hash(files: Sequence[Path]) -> Optional[str]:
    """First 16 hex digits of sha256 over the files' bytes, concatenated in
    order (the Makefile computes the same with `cat ... | sha256sum`); None
    when a source is absent (a library shipped without its sources)."""
    h = hashlib.sha256()
    for f in files:
        if not Path(f).is_file():
            return None
        h.update(Path(f).read_bytes())
    return h.hexdigest()[:16]


def embedded_hash(lib_path: Path, tag: bytes = b"nr-build-hash:") -> Optional[str]:
    """The build hash a library carries (read from its bytes, without loading it)."""
    try:
        data = Path(lib_path).read_bytes()
    except OSError:
        return None
    i = data.find(tag)
    return data[i + len(tag):i + len(tag) + 16].decode("ascii", "replace") if i >= 0 else None

NR_OK = 0
NR_F32 = 0
NR_BF16 = 1
NR_F16 = 2
NR_POOL_FINAL = 0
NR_POOL_LATENT = 1
NR_POOL_MEAN = 2
NR_POOL_NONE = -1
NR_EPI_NONE = 0
NR_EPI_RELU = 1
NR_EPI_EXP = 2
NR_EPI_GEGLU = 3
NR_EPI_RESADD = 4
NR_EPI_GELU = 5
NR_EPI_RELU_DROPOUT = 6
NR_EPI_DRELU = 7
NR_EPI_SOFTMAX64 = 8
NR_EPI_SOFTMAX64_BWD = 9

_p = ctypes.c_void_p
_i = ctypes.c_int
_l = ctypes.c_int64
_f = ctypes.c_float

# name -> (restype, argtypes); must match include/newsrec.h
SIGNATURES = {
    "nr_version": (_i, []),
    "nr_build_hash": (ctypes.c_char_p, []),
    "nr_init": (_i, [_i]),
    "nr_last_error": (ctypes.c_char_p, []),
    "nr_residency_flush": (_i, []),
    "nr_rccl_version": (_i, []),
    "nr_latent_train_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_latent_train_step": (_i, [_p, _p, _l, _p]),
    "nr_final_train_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_final_train_step": (_i, [_p, _p, _l, _p]),
    "nr_comm_unique_id": (_i, [_p]),
    "nr_comm_init": (_i, [_p, _p, _i, _i]),
    "nr_comm_init_timeout": (_i, [_p, _p, _i, _i, _l]),
    "nr_comm_destroy": (_i, [_p]),
    "nr_allgather": (_i, [_p, _p, _p, _l, _p]),
    "nr_is_device_pointer": (_i, [_p]),
    "nr_set_persistent_workgroups": (_i, [_i]),
    "nr_persistent_workgroups": (_i, []),
    "nr_set_gemm_half_tail": (_i, [_i]),
    "nr_gemm": (_i, [_i, _i, _i, _l, _l, _l, _p, _l, _p, _l, _p, _p, _l, _p, _l, _p]),
    "nr_gemm_relu_dropout": (_i, [_i, _i, _l, _l, _l, _p, _l, _p, _l, _p, _p, _l, ctypes.c_uint64, _f, _p]),
    "nr_gemm_drelu": (_i, [_i, _i, _l, _l, _l, _p, _l, _p, _l, _p, _l, _p, _l, _f, _p]),
    "nr_gemm_grouped": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "nr_gemm_grouped_tn": (_i, [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "nr_layernorm": (_i, [_i, _i, _l, _l, _p, _l, _p, _p, _f, _p, _l, _p]),
    "nr_gather_layernorm": (_i, [_i, _l, _l, _p, _l, _p, _i, _p, _p, _f, _p, _l, _p]),
    "nr_softmax64": (_i, [_l, _l, _p, _l, _i, _p, _l, _p]),
    "nr_row_inv_norm": (_i, [_i, _l, _l, _p, _l, _f, _p, _p]),
    "nr_pool_score": (_i, [_i, _i, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _l, _p, _p, _p]),
    "nr_score_users": (_i, [_i, _l, _p, _p, _p, _l, _p, _p, _p, _l, _p, _p]),
    "nr_splitk_fixup": (_i, [_i, _i, _l, _l, _i, _p, _p, _p, _l, _p, _l, _l, ctypes.c_uint64, _f, _f, _p]),
    "nr_dense_rank": (_i, [_p, _p, _l, _p, _p, _p]),
    "nr_impression_metrics": (_i, [_p, _p, _p, _l, _p, _p, _p, _p]),
    "nr_final_attn_workspace_bytes": (_l, [_i, _l]),
    "nr_final_attn_transform": (_i, [_i, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "nr_latent_workspace_bytes": (_l, [_i, _l]),
    "nr_latent_transform": (_i, [_i, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "nr_latent_transform_lnfold": (_i, [_i, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "nr_row_stats": (_i, [_i, _l, _l, _p, _l, _f, _p, _p]),
    "nr_embed_ln": (_i, [_i, _l, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p]),
    "nr_attention_varlen": (_i, [_i, ctypes.c_int32, _l, _p, _p, _p, _p, _p]),
    "nr_gather_rows": (_i, [_i, _i, _l, _l, _p, _l, _p, _p, _l, _p]),
    "nr_transpose": (_i, [_i, _i, _l, _l, _p, _l, _p, _l, _p]),
    "nr_final_pool_fwd": (_i, [_i, _l, _p, _p, _l, _p, _p, _p]),
    "nr_final_pool_bwd": (_i, [_i, _l, _p, _l, _p, _l, _p, _p, _p, _p, _l, _p, _l, _p]),
    "nr_cosine_margin": (_i, [_l, _p, _p, _l, _p, _p, _f, _p, _p, _p, _p, _p]),
    "nr_scatter_add_rows": (_i, [_i, _l, _l, _p, _l, _p, _p, _l, _p]),
    "nr_col_sum": (_i, [_i, _l, _l, _p, _l, _p, _p]),
    "nr_ln_param_grad": (_i, [_i, _l, _l, _p, _l, _p, _f, _p, _l, _p, _p, _p]),
    "nr_sumsq": (_i, [_l, _p, _p, _p]),
    "nr_layernorm_bwd": (_i, [_l, _l, _p, _l, _p, _f, _p, _l, _p, _l, _p, _l, _p]),
    "nr_softmax64_bwd": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _l, _p]),
    "nr_geglu_fwd": (_i, [_i, _l, _l, _p, _l, _p, _l, _p]),
    "nr_geglu_bwd": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _l, _p]),
    "nr_adamw": (_i, [_l, _p, _p, _p, _p, _p, _l, _f, _f, _f, _f, _f, _f, _p, _p]),
    "nr_encoder_workspace_bytes": (_l, [_i, _l, _l]),
    "nr_encoder_forward": (_i, [_i, _i, _p, _p, _l, _p, _l, _p, _p, _p, _f, _l, _l, _p, _p, _i, _p, _p, _p, _p, _l,
                                _p]),
}

# the InfoNCE entries (include/newsrec_contrastive.h), bound by load() like SIGNATURES
CONTRASTIVE_SIGNATURES = {
    "nr_cosine_infonce_workspace_bytes": (_l, [_l, _l]),
    "nr_cosine_infonce": (_i, [_l, _l, _p, _p, _l, _p, _p, _p, _f, _p, _p, _p, _p, _p, _l, _p]),
    "nr_final_train_step_contrastive_workspace_bytes": (_l, [_i, _l, _l, _l, _l]),
    "nr_final_train_step_contrastive": (_i, [_p, _p, _p, _l, _p]),
    "nr_latent_train_step_contrastive_workspace_bytes": (_l, [_i, _l, _l, _l, _l]),
    "nr_latent_train_step_contrastive": (_i, [_p, _p, _p, _l, _p]),
}

# top-K retrieval (include/newsrec_topk.h), bound by load() like SIGNATURES
NR_TOPK_MAX = 64
TOPK_SIGNATURES = {
    "nr_topk_chunk_rows": (_l, []),
    "nr_topk_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_topk_users": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _l, _p, _p, _p, _l, _p]),
}

# full-table ranks of target news (include/newsrec_fullrank.h), bound by load() like SIGNATURES
FULLRANK_SIGNATURES = {
    "nr_rank_targets_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_rank_targets": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _l, _p, _p, _p, _p, _l, _p]),
}

# MMR re-ranking of retrieved lists (include/newsrec_rerank.h), bound by load() like SIGNATURES
NR_RERANK_MAX = 64
RERANK_SIGNATURES = {
    "nr_rerank_mmr": (_i, [_i, _l, _l, _l, _p, _l, _p, _p, _p, _l, _l, _f, _p, _p, _p, _p, _p, _p]),
}

# per-click attribution of scores (include/newsrec_explain.h), bound by load() like SIGNATURES
NR_EXPLAIN_TOP_MAX = 8
EXPLAIN_SIGNATURES = {
    "nr_explain_scores": (_i, [_i, _i, _l, _p, _l, _l, _p, _l, _p, _l, _p, _p, _p, _l, _l, _p, _p, _p, _p, _p]),
}

# catalogue filters of retrieval and ranks (include/newsrec_filter.h), bound by load() like SIGNATURES
FILTER_SIGNATURES = {
    "nr_topk_users_filtered": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _l,
                                    _p]),
    "nr_rank_targets_filtered": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p,
                                      _l, _p]),
}

# sectioned top-K retrieval (include/newsrec_sections.h), bound by load() like SIGNATURES
NR_SECTIONS_MAX = 16
SECTIONS_SIGNATURES = {
    "nr_topk_sections_workspace_bytes": (_l, [_i, _l, _l, _l, _l]),
    "nr_topk_sections": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _l, _l, _p, _p, _p, _l,
                              _p]),
}

# the rank-one prior of retrieval, ranks and sections (include/newsrec_prior.h), bound by load() like
# SIGNATURES: the filtered / sectioned entries' arguments with news_prior and user_gain behind the
# mask pointer and top_keys behind top_scores
PRIOR_SIGNATURES = {
    "nr_topk_users_prior_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_topk_users_prior": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p,
                                 _p, _l, _p]),
    "nr_rank_targets_prior_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_rank_targets_prior": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _p, _p,
                                   _p, _p, _l, _p]),
    "nr_topk_sections_prior_workspace_bytes": (_l, [_i, _l, _l, _l, _l]),
    "nr_topk_sections_prior": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _l, _p,
                                    _p, _p, _p, _l, _p]),
}

# column-sliced pool+score (include/newsrec_sliced.h), bound by load() like SIGNATURES
SLICED_SIGNATURES = {
    "nr_slice_table": (_i, [_i, _l, _i, _i, _p, _l, _p, _i, _p]),
    "nr_pool_score_sliced_workspace_bytes": (_l, [_i, _l, _l]),
    "nr_pool_score_sliced": (_i, [_i, _i, _l, _i, _p, _l, _p, _l, _p, _p, _p, _p, _p, _l, _l, _p, _p, _l, _p]),
}

# per-group caps of retrieval (include/newsrec_caps.h), bound by load() like SIGNATURES:
# nr_topk_users_prior's arguments with news_group and cap behind user_gain
NR_CAP_GROUPS_MAX = 1024
CAPS_SIGNATURES = {
    "nr_topk_users_capped_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_topk_users_capped": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _l, _p,
                                  _p, _p, _p, _l, _p]),
}

# cursors of retrieval (include/newsrec_page.h), bound by load() like SIGNATURES: nr_topk_users_prior's
# arguments with after_key, after_row, next_key and next_row behind user_gain
NR_DEEP_MAX = 1024  # the longest list PoolScoreEngine.recommend_deep pages to
PAGE_SIGNATURES = {
    "nr_topk_users_after_workspace_bytes": (_l, [_i, _l, _l, _l]),
    "nr_topk_users_after": (_i, [_i, _l, _l, _p, _l, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                 _l, _p, _p, _p, _p, _l, _p]),
}

# deep retrieval (include/newsrec_deep.h), bound by load() like SIGNATURES: nr_topk_users_after's
# arguments, K up to NR_TOPK_DEEP_MAX from one walk over the table
NR_TOPK_DEEP_MAX = 256
DEEP_SIGNATURES = {
    "nr_topk_users_deep_workspace_bytes": PAGE_SIGNATURES["nr_topk_users_after_workspace_bytes"],
    "nr_topk_users_deep": PAGE_SIGNATURES["nr_topk_users_after"],
}

# the request path of retrieval (include/newsrec_request.h), bound by load() like SIGNATURES:
# nr_topk_users_after's arguments for at most NR_REQUEST_MAX_USERS users
NR_REQUEST_MAX_USERS = 32
REQUEST_SIGNATURES = {
    "nr_topk_request_run_rows": (_l, [_l]),
    "nr_topk_request_workspace_bytes": PAGE_SIGNATURES["nr_topk_users_after_workspace_bytes"],
    "nr_topk_request": PAGE_SIGNATURES["nr_topk_users_after"],
}


class ContrastiveSpec(ctypes.Structure):
    """struct nr_contrastive_spec (include/newsrec_contrastive.h)."""
    _fields_ = [("Cn", _l), ("cand", _p), ("target", _p), ("mask", _p), ("inv_tau", _f)]


class EncoderLayer(ctypes.Structure):
    """struct nr_encoder_layer (include/newsrec.h): device pointers of one layer."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("wqkv", "bqkv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2",
                                             "ln2_g", "ln2_b")]


LATENT_TRAIN_PARAMS = ("tok_g", "tok_b", "latents", "nq_g", "nq_b", "nc_g", "nc_b", "Wq", "Wkv", "Wo", "nf_g", "nf_b",
                       "W1", "b1", "W2", "b2")
LATENT_TRAIN_GRADS = tuple("g_" + n for n in LATENT_TRAIN_PARAMS)
FINAL_TRAIN_PARAMS = ("tok_g", "tok_b", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5")
FINAL_TRAIN_GRADS = tuple("g_" + n for n in FINAL_TRAIN_PARAMS)


def _train_fields(params, grads, extra_fields=()) -> list:
    """Fields of a train step's args struct: the batch head both steps share, the
    step's own scalars (``extra_fields``, after ``margin``), then its parameter,
    gradient and output pointers."""
    ptrs = lambda names: [(n, _p) for n in names]
    return ([("dtype", _i), ("tok_dtype", _i), ("B", _l), ("U", _l), ("Hs", _l)]
            + ptrs(("tok_last", "hist_idx", "hist_off", "pos", "neg")) + [("margin", _f)] + list(extra_fields)
            + ptrs(tuple(params) + tuple(grads) + ("loss", "users", "sumsq")))


class LatentTrainArgs(ctypes.Structure):
    """struct nr_latent_train_args (include/newsrec.h)."""
    _fields_ = _train_fields(LATENT_TRAIN_PARAMS, LATENT_TRAIN_GRADS)


class FinalTrainArgs(ctypes.Structure):
    """struct nr_final_train_args (include/newsrec.h)."""
    _fields_ = _train_fields(FINAL_TRAIN_PARAMS, FINAL_TRAIN_GRADS, [("p", _f), ("seed", ctypes.c_uint64 * 3)])


class NewsRecHIPError(RuntimeError):
    """A libnewsrec_hip call failed (or the library is not available)."""


_LIB = None


def load() -> ctypes.CDLL:
    """Load the HIP library once; raise loudly if it was not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.is_file():
        raise NewsRecHIPError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the MI355X hot path)")
    lib = ctypes.CDLL(os.fspath(LIB_PATH))
    for name, (res, args) in {**SIGNATURES, **CONTRASTIVE_SIGNATURES, **TOPK_SIGNATURES,
                              **FULLRANK_SIGNATURES, **RERANK_SIGNATURES, **EXPLAIN_SIGNATURES,
                              **FILTER_SIGNATURES, **SECTIONS_SIGNATURES, **PRIOR_SIGNATURES,
                              **CAPS_SIGNATURES, **PAGE_SIGNATURES, **SLICED_SIGNATURES,
                              **DEEP_SIGNATURES, **REQUEST_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    want = source_hash(hip_source_files())
    got = lib.nr_build_hash().decode("ascii", "replace")
    if want is not None and got != want:
        raise NewsRecHIPError(
            f"{LIB_PATH} was built from other sources (build hash {got}, tree {want}): rebuild it with "
            "`python -c 'import __graft_entry__ as g; g.build()'`")
    _LIB = lib
    return lib


def check(rc: int, name: str) -> None:
    if rc != NR_OK:
        msg = load().nr_last_error().decode(errors="replace")
        raise NewsRecHIPError(f"{name} failed ({rc}): {msg}")


def call(name: str, *args) -> None:
    check(getattr(load(), name)(*args), name)


def empty_cache() -> None:
    """torch.cuda.empty_cache() + nr_residency_flush(): the segments torch
    returns to the driver may be re-mapped later, so the library's cached
    "verified device range" tables are dropped with them (include/newsrec.h)."""
    import torch
    torch.cuda.empty_cache()
    if _LIB is not None:
        _LIB.nr_residency_flush()
