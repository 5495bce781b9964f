"""CPU reference (test support) of the InfoNCE loss of the config-5 steps: the
oracle's forwards (oracle/train_ref.py, oracle/pool_ref.py) composed with

    E_c  = LN_tok(tok_last[cand[c]])
    s_bc = cos(u_b, E_c)                      F.cosine_similarity's per-vector 1e-8 clamp
    z_bc = s_bc / tau, -inf where cand[c] < 0 or mask[b][c]
    loss = CrossEntropyLoss()(z, target)      mean over the B rows

in torch under autograd.  The sampled form with tau = 1 is the reference's commented
loss (trainer.py:612-625): ``res = cosine_similarity(outputs[rev].unsqueeze(1),
emb[news_ind_pos_neg], dim=-1); res[news_ind_pos_neg < 0] = -inf;
CrossEntropyLoss()(res, zeros)``.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pool_ref, train_ref


def infonce_logits(users, E, cand, mask, inv_tau):
    """z [B, Cn] (users [B, D], E [U, D] torch; cand [Cn] ints, -1 = pad; mask None or [B, Cn])."""
    c = torch.as_tensor(np.asarray(cand, dtype=np.int64))
    Ec = E[c.clamp(min=0)]
    z = F.cosine_similarity(users[:, None, :], Ec[None, :, :], dim=-1) * inv_tau
    excl = (c < 0)[None, :].expand(z.shape)
    if mask is not None:
        excl = excl | torch.as_tensor(np.asarray(mask)).bool()
    return z.masked_fill(excl, float("-inf"))


def infonce_loss(users, E, cand, target, mask, inv_tau):
    z = infonce_logits(users, E, cand, mask, inv_tau)
    return F.cross_entropy(z, torch.as_tensor(np.asarray(target, dtype=np.int64)))


def sampled_spec(pos_neg: np.ndarray):
    """(cand, target, mask) of the sampled form for a [B, 1 + K] block (indices into U, -1 pads)."""
    B, w = pos_neg.shape
    cand = np.asarray(pos_neg, dtype=np.int32).ravel()
    mask = np.ones((B, B * w), dtype=np.uint8)
    for b in range(B):
        mask[b, b * w:(b + 1) * w] = 0
    return cand, (np.arange(B) * w).astype(np.int32), mask


def pooled_users(P, tok_last, hist_groups, pooler="final", numerics="f32", p=0.0, seeds=(0, 0, 0), ln_eps=1e-12):
    """(users [B, D], E [U, D]) as oracle.train_ref._loss forms them before its margin loss."""
    E = F.layer_norm(tok_last.to(P["ln.weight"].dtype), (tok_last.shape[1],), P["ln.weight"], P["ln.bias"], ln_eps)
    B = len(hist_groups)
    L = max(len(h) for h in hist_groups)
    idx = torch.zeros((B, L), dtype=torch.long)
    mask = torch.zeros((B, L), dtype=torch.int32)
    slot_rows = -np.ones((B, L), dtype=np.int64)
    r = 0
    for b, h in enumerate(hist_groups):
        idx[b, :len(h)] = torch.as_tensor(np.asarray(h, dtype=np.int64))
        mask[b, :len(h)] = 1
        slot_rows[b, :len(h)] = np.arange(r, r + len(h))
        r += len(h)
    second = E[idx] * mask.unsqueeze(-1)
    if pooler == "latent":
        lsd = {k[7:]: v for k, v in P.items() if k.startswith("latent.")}
        out = (train_ref.latent_attention_train_bf16(lsd, second, mask) if numerics == "bf16" else
               pool_ref.latent_attention_forward(lsd, second, mask))
    elif numerics == "bf16":
        out = train_ref.final_attention_train_bf16(P, second, mask)
    else:
        out = train_ref.final_attention_train(P, second, mask, seeds, p, slot_rows)
    return out, E


def contrastive_step(params: dict, tok_last, hist_groups, cand, target, mask, *, temperature=1.0, pooler="final",
                     numerics="f32", ln_eps=1e-12, dtype=torch.float32):
    """Loss and gradients of one contrastive step (dropout off): dict(loss, grads, users)."""
    P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    users, E = pooled_users(P, tok_last.to(dtype), hist_groups, pooler, numerics, ln_eps=ln_eps)
    loss = infonce_loss(users, E, cand, target, mask, 1.0 / temperature)
    loss.backward()
    return {"loss": float(loss.detach()), "users": users.detach(),
            "grads": {k: v.grad.detach().clone() for k, v in P.items() if v.grad is not None}}


def contrastive_epoch(params: dict, batches, *, temperature=1.0, pooler="final", lr=1e-6, max_norm=0.5,
                      weight_decay=0.01, ln_eps=1e-12):
    """The train_one_epoch loop with the InfoNCE loss and ONE persistent AdamW over
    ``batches`` = [(tok_last, hist_groups, cand, target, mask, n_rows)]: (row-weighted
    mean loss, params after)."""
    P = {k: v.detach().clone().float().requires_grad_(True) for k, v in params.items()}
    plist = list(P.values())
    opt = torch.optim.AdamW(plist, lr=lr, weight_decay=weight_decay)
    tot, cnt = 0.0, 0
    for tok_last, groups, cand, target, mask, n in batches:
        opt.zero_grad()
        users, E = pooled_users(P, tok_last, groups, pooler, ln_eps=ln_eps)
        loss = infonce_loss(users, E, cand, target, mask, 1.0 / temperature)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([q for q in plist if q.grad is not None], max_norm=max_norm)
        opt.step()
        tot += float(loss.detach()) * n
        cnt += n
    return tot / cnt, {k: v.detach().clone() for k, v in P.items()}
