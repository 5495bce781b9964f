"""Glue between the data layer and the poolers (reference data_model_helper.py).

Same signatures and return types as the reference functions of the hot path;
the work runs on the MI355X through ``PoolScoreEngine``:
  reference (CPU/GPU torch)                           here (HIP)
  pad each batch to its longest history, run the      per-news transform once
  pooler on every padded slot, mask  (:112-131)       (MFMA GEMM chain) + segmented
  per-impression F.cosine_similarity loop (:199-230)  pool+score kernel, one launch
  rankdata per impression (:442, data_utils:414)      nr_dense_rank kernel
"""
from __future__ import annotations

from typing import Iterable, Optional

import numpy as np
import torch

from .config import DEVICE
from .data_utils import group_items
from .engine import PoolScoreEngine

# Compute dtype of the table/GEMM path.  float32 is the parity configuration
# (scores within 1e-4 of the reference); bfloat16 is BASELINE config 3.
COMPUTE_DTYPE = torch.float32

# Phase split of the last get_final_second_attention_score call (ms), filled
# when PROFILE is set: setup_upload (engine and pooler weights, the news table
# and the CSR index arrays host -> HBM),
# device (transform + pool + score + dense ranks), download (scores + ranks),
# host (grouping into per-impression arrays).  PROFILE adds a device sync
# between the phases; off, the call syncs only where it returns host data.
PROFILE = False
LAST_TIMINGS: dict = {}


class _Phases:
    def __init__(self):
        import time
        self._clock = time.perf_counter
        self.t = self._clock()
        self.out = {}

    def mark(self, name: str, sync: bool = True) -> None:
        if not PROFILE:
            return
        if sync and torch.cuda.is_available():
            torch.cuda.synchronize()
        now = self._clock()
        self.out[name] = (now - self.t) * 1e3
        self.t = now

    def publish(self) -> None:
        if PROFILE:
            LAST_TIMINGS.clear()
            LAST_TIMINGS.update({k: round(v, 3) for k, v in self.out.items()})
            LAST_TIMINGS["total"] = round(sum(self.out.values()), 3)


def _host(t: torch.Tensor) -> np.ndarray:
    """Device tensor -> numpy array backed by pinned host memory (torch's caching
    host allocator; the array keeps its block alive): one DMA at the PCIe rate,
    56 GB/s for the MIND-large-dev scores against 6.5 GB/s for the pageable
    `.cpu()` (tools/pcie_probe.py, profiles/round6/pcie_probe.jsonl)."""
    if t.device.type != "cuda":
        return t.numpy()
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return out.numpy()


def _engine(model, news_embeddings, query_news_embeddings=None, dtype=None) -> PoolScoreEngine:
    eng = PoolScoreEngine(model, dtype=dtype or COMPUTE_DTYPE, device=DEVICE)
    eng.load_news(news_embeddings, query_news_embeddings)
    return eng


def get_final_attention_eval(history_rev_index: np.ndarray, history_len_list: np.ndarray,
                             news_embeddings: torch.Tensor, model: torch.nn.Module, dtype=None) -> torch.Tensor:
    """Pooled user vectors [I', D] on the host (data_model_helper.py:112-131)."""
    eng = _engine(model, news_embeddings, dtype=dtype)
    n = len(history_len_list)
    eng.load_impressions(history_rev_index, history_len_list, np.zeros(0, np.int32), np.zeros(n, np.int32))
    eng.hist_table = eng.transform()
    eng.inv_norms()
    _, users = eng.pool_score(want_users=True)
    return users.cpu()


def get_cos_sim_scores(history_rev_index: np.ndarray, history_len_list: np.ndarray, news_rev_index: np.ndarray,
                       impression_len_list: np.ndarray, news_embeddings: torch.Tensor, model: torch.nn.Module,
                       query_news_embeddings: Optional[torch.Tensor] = None, dtype=None) -> torch.Tensor:
    """Cosine score of every candidate against its impression's pooled history,
    impression-major [C] f32 on the host (data_model_helper.py:174-239)."""
    assert len(history_len_list) == len(impression_len_list), "Number of rows should be consistent"
    assert sum(impression_len_list) == len(news_rev_index), \
        "Number of impressions should match length of impression list"
    eng = _engine(model, news_embeddings, query_news_embeddings if isinstance(query_news_embeddings, torch.Tensor)
                  else None, dtype=dtype)
    eng.load_impressions(history_rev_index, history_len_list, news_rev_index, impression_len_list)
    scores, _ = eng.step()
    return torch.from_numpy(_host(scores))


def get_final_second_attention_score(history_rev_index: np.ndarray, history_len_list: np.ndarray,
                                     news_rev_index: np.ndarray, impression_len_list: np.ndarray,
                                     news_embeddings: torch.Tensor, history_bool, attention_model: torch.nn.Module,
                                     dtype=None) -> dict:
    """Scores of the impressions that have a history, then dense ranks per
    impression (data_model_helper.py:416-443).

    As in the reference, ``grouped_scores`` groups by the UNFILTERED
    ``impression_len_list`` (consistent under DataSubset.WITH_HISTORY).
    """
    hb = np.asarray(history_bool, dtype=bool)
    imp_len = np.asarray(impression_len_list)
    cand_keep = np.repeat(hb, imp_len)
    sub_news = np.asarray(news_rev_index)[cand_keep]
    sub_len = imp_len[hb]
    assert len(history_len_list) == len(sub_len), "Number of rows should be consistent"
    ph = _Phases()
    eng = _engine(attention_model, news_embeddings, dtype=dtype)
    eng.load_impressions(history_rev_index, history_len_list, sub_news, sub_len)
    ph.mark("setup_upload")
    scores_d, _ = eng.step()
    ranks_d = eng.rank(scores_d) if hb.all() else None
    ph.mark("device")
    scores = _host(scores_d)
    ranks = _host(ranks_d) if ranks_d is not None else None
    ph.mark("download")
    if ranks is not None:
        grouped = group_items(ranks.astype(np.int64), imp_len)
    else:  # reference quirk: grouping by the unfiltered lengths
        from .data_utils import rank_group_preds
        grouped = rank_group_preds(scores, imp_len)
    ph.mark("host", sync=False)
    ph.publish()
    return {"scores": scores, "grouped_scores": grouped}


def _check_prior_args(what: str, prior, prior_gain, n_news: int, n_imp: int, reranked: bool) -> None:
    """The prior arguments of the retrieval helpers, refused before any device work."""
    from .engine import check_gain, check_prior
    if prior is not None:
        check_prior(prior, n_news)
    if prior_gain is None:
        return
    if prior is None:
        raise ValueError(f"{what}: prior_gain needs prior")
    check_gain(prior_gain, n_imp)
    if reranked:
        raise ValueError(f"{what}: prior_gain cannot be combined with diversify or explain")


def get_top_k_recommendations(history_rev_index: np.ndarray, history_len_list: np.ndarray,
                              news_embeddings: torch.Tensor, attention_model: torch.nn.Module, k: int,
                              exclude_history: bool = True, query_news_embeddings: Optional[torch.Tensor] = None,
                              dtype=None, diversify: Optional[float] = None, pool: Optional[int] = None,
                              news_time=None, news_category=None, time_window=None, categories=None,
                              sections=None, prior=None, prior_gain=None, groups=None, group_cap=None,
                              page: Optional[int] = None, walk: Optional[int] = None,
                              explain: Optional[int] = None) -> dict:
    """The k news of the WHOLE table that the model recommends per impression:
    ``{"news_index": int32 [I, k], "scores": float32 [I, k]}`` on the host, score
    descending, ties by ascending news row, ``(-1, -inf)`` where fewer than k news are
    eligible.  The scores are get_cos_sim_scores' for that (impression, news) pair.
    ``exclude_history`` leaves an impression's own history out of its list (the history
    rows are taken as rows of ``news_embeddings``).

    The reference has no counterpart: it only scores the candidates an impression
    lists.  This is PoolScoreEngine.recommend (users x table as one MFMA GEMM with
    the K best kept per user as the tiles are produced, include/newsrec_topk.h).

    ``diversify`` = lambda in [0, 1] re-ranks for diversity (PoolScoreEngine.recommend_diverse,
    greedy MMR, include/newsrec_rerank.h): the ``pool`` (default 64, at least k) best news
    are retrieved and k of them picked one at a time, each maximising lambda * score -
    (1 - lambda) * (largest cosine to a news already picked).  The lists are then in
    pick order, the scores still the news' own, and the result gains ``"ild"`` float32
    [I, 2], the intra-list diversity of the plain top-k list and of the returned one, and
    ``"plain_scores"`` float32 [I, k], the plain top-k list's scores
    (evaluation.diversity_metrics summarises them).  ``pool`` without ``diversify`` is refused.

    ``explain`` = T in [1, 8] adds the reasons (PoolScoreEngine.recommend_explained,
    include/newsrec_explain.h): ``"why_news"`` int32 [I, k, T], for each recommendation the T
    news of the impression's history (rows of the news table) whose clicks contributed
    most to its score, and ``"why_share"`` float32 [I, k, T], those clicks' additive shares
    of the score (all of a history's shares add up to the score), value descending;
    ``(-1, -inf)`` for a missing recommendation and past the history's length
    (evaluation.explanation_metrics summarises them).  Without ``explain`` the result is as
    described above.

    Catalogue filters (include/newsrec_filter.h): ``news_time`` int32 [N] with ``time_window``
    = (lo, hi) keeps the news with lo <= news_time <= hi, ``news_category`` [N] ids (0 .. 63)
    with ``categories`` = a 64-bit mask keeps the news whose category's bit is set; window
    and mask are scalars or one value per impression.  Every mode above then draws from the
    eligible news only.

    ``sections`` = a sequence of disjoint sections, each a 64-bit category mask or an iterable
    of category ids (0 .. 63), builds a front page (PoolScoreEngine.recommend_sections,
    include/newsrec_sections.h): ``news_index`` and ``scores`` are then [I, S, k], the k best
    eligible news of each section from one walk over the table, and ``k`` means per section
    (S <= 16, S * k <= 64).  It needs ``news_category`` and composes with ``time_window``;
    with ``categories``, ``diversify`` or ``explain`` it is refused.

    ``prior`` f32 [N] (finite; e.g. data_utils.history_popularity) with ``prior_gain`` = g, a
    finite scalar or one value per impression, selects and orders the news by ``score + g *
    prior`` (PoolScoreEngine.recommend's ``prior_gain``, include/newsrec_prior.h): g = 0 changes
    nothing, an impression with an empty history gets the news with the largest prior.  The
    ``scores`` stay the cosines and the result gains ``"keys"`` float32, shaped like them: what
    the lists are ordered by.  It composes with the catalogue filters and ``sections``; with
    ``diversify`` or ``explain`` it is refused.

    ``groups`` [N] integer labels in [0, 1024) (data_utils.dense_groups makes them from category
    names, sub-categories, publishers ...) with ``group_cap`` = c in 1 .. 64 allows at most c
    news of one group in a list (PoolScoreEngine.recommend's ``group_cap``,
    include/newsrec_caps.h): the eligible news are walked best first and one is taken while
    its group holds fewer than c, so a list may end in ``(-1, -inf)`` before k.  Both or
    neither; it composes with the catalogue filters and the prior (the result then has
    ``"keys"``), and is refused with ``sections``, ``diversify`` and ``explain``.

    ``page`` = P in 1 .. 64 lifts the limit on k from 64 to 1024 (PoolScoreEngine.recommend_deep,
    include/newsrec_page.h): the list is fetched in ceil(k / P) cursor calls of P rows, each
    continuing exactly where the one before ended, and returned ordered by score (by key
    under a prior) descending, ties by ascending news row.  It composes with the catalogue
    filters and the prior, and is refused with ``sections``, ``diversify``, ``explain`` and
    ``group_cap``.  Without ``page`` nothing changes: k > 64 is refused.

    ``walk`` = W in 1 .. 256 lifts the limit on k to 1024 as ``page`` does, and returns the same
    lists bit for bit (PoolScoreEngine.recommend_deep(walk=W), include/newsrec_deep.h): the list
    is fetched in ceil(k / W) chained calls of W rows that each need one walk over the table,
    where a page of 64 needs one per 64 rows.  ``walk`` and ``page`` are mutually exclusive, and
    ``walk`` is refused with ``sections``, ``diversify``, ``explain`` and ``group_cap``."""
    if walk is not None:
        if page is not None:
            raise ValueError("get_top_k_recommendations: walk and page are mutually exclusive")
        if (sections is not None or diversify is not None or explain is not None or pool is not None
                or group_cap is not None or groups is not None):
            raise ValueError("get_top_k_recommendations: walk cannot be combined with sections, diversify, explain "
                             "or group_cap")
        from .engine import PAGE_MAX, check_deep
        check_deep("get_top_k_recommendations", k, PAGE_MAX, walk)
    elif page is not None:
        if (sections is not None or diversify is not None or explain is not None or pool is not None
                or group_cap is not None or groups is not None):
            raise ValueError("get_top_k_recommendations: page cannot be combined with sections, diversify, explain "
                             "or group_cap")
        from .engine import check_deep
        check_deep("get_top_k_recommendations", k, page)
    elif sections is None and diversify is None and explain is None and pool is None and not 1 <= k <= 64:
        from . import ops  # the entry's own refusal, ahead of any device work
        ops.topk_workspace_bytes(torch.float32 if dtype is None else dtype, 1, news_embeddings.shape[0], k)
    if (groups is None) != (group_cap is None):
        raise ValueError("get_top_k_recommendations: groups and group_cap go together")
    if group_cap is not None:
        if sections is not None or diversify is not None or explain is not None or pool is not None:
            raise ValueError("get_top_k_recommendations: group_cap cannot be combined with sections, diversify or "
                             "explain")
        from .engine import check_groups
        check_groups(groups, news_embeddings.shape[0])  # bad labels are refused before any device work
        if isinstance(group_cap, bool) or not isinstance(group_cap, (int, np.integer)) or not 1 <= group_cap <= 64:
            raise ValueError(f"get_top_k_recommendations: group_cap = {group_cap!r} must be an integer in 1 .. 64")
    _check_prior_args("get_top_k_recommendations", prior, prior_gain, news_embeddings.shape[0],
                      len(history_len_list), diversify is not None or explain is not None or pool is not None)
    if sections is not None:
        if categories is not None or diversify is not None or explain is not None or pool is not None:
            raise ValueError("get_top_k_recommendations: sections cannot be combined with categories, diversify or "
                             "explain")
        from .engine import section_masks
        section_masks(sections)  # a bad item is refused before any device work
        if news_category is None:
            raise ValueError("get_top_k_recommendations: sections needs news_category")
        if time_window is not None and news_time is None:
            raise ValueError("get_top_k_recommendations: time_window needs news_time")
    if diversify is None and pool is not None:
        raise ValueError("get_top_k_recommendations: pool needs diversify")
    if explain is not None and not 1 <= int(explain) <= 8:
        raise ValueError(f"get_top_k_recommendations: explain = {explain} outside [1, 8]")
    eng = _engine(attention_model, news_embeddings, query_news_embeddings if isinstance(query_news_embeddings,
                                                                                        torch.Tensor) else None,
                  dtype=dtype)
    n = len(history_len_list)
    eng.load_impressions(history_rev_index, history_len_list, np.zeros(0, np.int32), np.zeros(n, np.int32))
    if sections is not None:
        eng.set_catalogue(news_time=news_time, news_cat=news_category, news_prior=prior)
        if prior_gain is not None:
            idx, scores, keys = eng.recommend_sections(k, sections, exclude_history=exclude_history,
                                                       time_window=time_window, prior_gain=prior_gain, want_keys=True)
            return {"news_index": _host(idx), "scores": _host(scores), "keys": _host(keys)}
        idx, scores = eng.recommend_sections(k, sections, exclude_history=exclude_history, time_window=time_window)
        return {"news_index": _host(idx), "scores": _host(scores)}
    flt = {}
    if time_window is not None or categories is not None or prior_gain is not None or group_cap is not None:
        eng.set_catalogue(news_time=news_time, news_cat=news_category, news_prior=prior, news_group=groups)
        flt = {"time_window": time_window, "categories": categories}
    if page is not None or walk is not None:
        deep = {"page": int(page)} if walk is None else {"walk": int(walk)}
        idx, scores, keys = eng.recommend_deep(int(k), exclude_history=exclude_history, prior_gain=prior_gain,
                                               want_keys=True, **deep, **flt)
        res = {"news_index": _host(idx), "scores": _host(scores)}
        return {**res, "keys": _host(keys)} if prior_gain is not None else res
    if group_cap is not None:
        idx, scores, keys = eng.recommend(k, exclude_history=exclude_history, prior_gain=prior_gain, want_keys=True,
                                          group_cap=int(group_cap), **flt)
        res = {"news_index": _host(idx), "scores": _host(scores)}
        return {**res, "keys": _host(keys)} if prior_gain is not None else res
    if prior_gain is not None:
        idx, scores, keys = eng.recommend(k, exclude_history=exclude_history, prior_gain=prior_gain, want_keys=True,
                                          **flt)
        return {"news_index": _host(idx), "scores": _host(scores), "keys": _host(keys)}
    why = {}
    if explain is not None:
        explained = eng.recommend_explained_filtered if flt else eng.recommend_explained
        idx, scores, why_news, why_val = explained(k, top=int(explain), lam=diversify,
                                                   pool=64 if pool is None else pool,
                                                   exclude_history=exclude_history, **flt)
        why = {"why_news": _host(why_news), "why_share": _host(why_val)}
        if diversify is None:
            return {"news_index": _host(idx), "scores": _host(scores), **why}
    if diversify is not None:
        idx, scores, ild, plain = eng.recommend_diverse(k, diversify, pool=64 if pool is None else pool,
                                                        exclude_history=exclude_history, want_ild=True,
                                                        want_plain=True, **flt)
        return {"news_index": _host(idx), "scores": _host(scores), "ild": _host(ild), "plain_scores": _host(plain),
                **why}
    idx, scores = eng.recommend(k, exclude_history=exclude_history, **flt)
    return {"news_index": _host(idx), "scores": _host(scores)}


def get_full_table_ranks(history_rev_index: np.ndarray, history_len_list: np.ndarray, target_index: np.ndarray,
                         target_len_list: np.ndarray, news_embeddings: torch.Tensor, attention_model: torch.nn.Module,
                         exclude_history: bool = True, query_news_embeddings: Optional[torch.Tensor] = None,
                         dtype=None, news_time=None, news_category=None, time_window=None,
                         categories=None, prior=None, prior_gain=None) -> dict:
    """Where the given news stand among ALL news of the table for each impression's
    user: ``{"ranks": int32 [T]}`` on the host, in the order of ``target_index``
    (``target_len_list[i]`` rows of ``news_embeddings`` for impression i, e.g. its
    clicked candidates).  A rank is the number of eligible news the model puts before
    the target (score descending, ties by ascending news row): 0 is the top
    recommendation, and the targets with rank < k are exactly the rows
    get_top_k_recommendations returns for that k.  -1 marks a target that is in the
    impression's own history (with ``exclude_history``) or outside the table.
    evaluation.retrieval_metrics turns the ranks into hit / recall / nDCG@K, MRR and
    the mean and median rank against the whole catalogue.

    The reference has no counterpart: its AUC / MRR / nDCG are taken over the handful
    of candidates an impression lists.  This is PoolScoreEngine.rank_targets (the
    users x table MFMA product of the top-K path with a counting epilogue,
    include/newsrec_fullrank.h).  ``news_time`` / ``news_category`` / ``time_window`` /
    ``categories`` are get_top_k_recommendations' catalogue filters: only the eligible news
    are counted, and a target its impression's filter leaves out gets -1.  ``prior`` /
    ``prior_gain`` are get_top_k_recommendations' too: the ranks are then taken on ``score + g *
    prior``, and the targets with rank < k are the rows it returns under the same arguments."""
    _check_prior_args("get_full_table_ranks", prior, prior_gain, news_embeddings.shape[0], len(history_len_list),
                      False)
    eng = _engine(attention_model, news_embeddings, query_news_embeddings if isinstance(query_news_embeddings,
                                                                                        torch.Tensor) else None,
                  dtype=dtype)
    n = len(history_len_list)
    eng.load_impressions(history_rev_index, history_len_list, np.zeros(0, np.int32), np.zeros(n, np.int32))
    flt = {}
    if time_window is not None or categories is not None or prior_gain is not None:
        eng.set_catalogue(news_time=news_time, news_cat=news_category, news_prior=prior)
        flt = {"time_window": time_window, "categories": categories, "prior_gain": prior_gain}
    return {"ranks": _host(eng.rank_targets(target_index, target_len_list, exclude_history=exclude_history, **flt))}


def get_embeddings(model_path: str, news_list: Iterable[str], news_text_dict: dict[str, str]):
    """Title encoder entry (data_model_helper.py:45-84): see encoder.py."""
    from .encoder import get_embeddings as _ge
    return _ge(model_path, news_list, news_text_dict)


def apply_token_attn(model_path, db_name, num_samples: int) -> torch.Tensor:
    """Token-attention table of news 0..num_samples-1 from the sqlite token DB
    (data_model_helper.py:390-413): ``FirstAttentionPoolFunc(last_token_pool)``
    per news -> [N, D] f32 on the host.

    The reference pads each batch of token states, ships them to the device and
    runs the (dead) attention; its output is the g_mlp_layernorm chain of each
    news' last valid token (attention.py:193, modeling_utils.py:37-48), so only
    those rows are uploaded and the LN runs in ``nr_gather_layernorm``."""
    import sqlite3

    from .data_utils import iter_token_states
    from .modeling_utils import get_token_attn_model
    model = get_token_attn_model(model_path)
    out = []
    with sqlite3.connect(str(db_name)) as conn:
        for rows, lens in iter_token_states(conn, num_samples):
            last = rows[torch.as_tensor(np.cumsum(lens) - 1)]
            dev_rows = last.to(DEVICE).contiguous()
            seg = torch.arange(len(lens) + 1, dtype=torch.int64, device=DEVICE)
            out.append(model.forward_packed(dev_rows, seg).cpu())
    return torch.cat(out) if out else torch.zeros((0, 1024))


def store_embeddings(model_path: str, news_list: Iterable[str], news_text_dict: dict[str, str], db_name,
                     dtype: torch.dtype = torch.float32) -> int:
    """Per-token title hidden states -> sqlite token DB (data_model_helper.py:374-387),
    with the MI355X title encoder on a LOCAL model directory."""
    from transformers import AutoTokenizer

    from .config import NEWS_TEXT_MAXLEN
    from .encoder import XLMREncoder, store_token_states, tokenize
    tok = AutoTokenizer.from_pretrained(model_path)
    enc = XLMREncoder.from_pretrained_dir(model_path, dtype=dtype)
    texts = [news_text_dict[n] for n in news_list]
    return store_token_states(enc, *tokenize(tok, texts, NEWS_TEXT_MAXLEN), db_name)


# The classification-baseline blend and the reduce-model experiments
# (data_model_helper.py:87-109, 134-171, 242-371) are outside the hot path
# (SURVEY §8(f)4): import-level placeholders only; calling one raises.
from .out_of_scope import placeholder_function as _oos  # noqa: E402

get_reduced_dim_embeds = _oos("get_reduced_dim_embeds", "data_model_helper.py:87-88", __name__)
get_classification_preds = _oos("get_classification_preds", "data_model_helper.py:91-98", __name__)
get_classification_baseline_scores = _oos("get_classification_baseline_scores", "data_model_helper.py:101-109",
                                          __name__)
get_cos_sim_reduce_scores = _oos("get_cos_sim_reduce_scores", "data_model_helper.py:134-171", __name__)
get_cos_sim_final_score = _oos("get_cos_sim_final_score", "data_model_helper.py:242-269", __name__)
get_final_score = _oos("get_final_score", "data_model_helper.py:272-301", __name__)
get_final_only_attention_score = _oos("get_final_only_attention_score", "data_model_helper.py:304-335", __name__)
get_final_only_reduce_attention_score = _oos("get_final_only_reduce_attention_score", "data_model_helper.py:338-371",
                                             __name__)
