/*
 * InfoNCE loss with in-batch negatives for the config-5 train steps (part of the
 * C ABI of libnewsrec_hip.so; included by newsrec.h's users next to it, same
 * error model: NR_OK or a negative code, message in nr_last_error()).
 *
 * A batch has B rows with pooled users u_b, a candidate list cand[Cn] (indices
 * into the batch's U unique news, -1 = pad column), target[B] (the column of row
 * b's positive) and a nullable mask [B][Cn] (uint8 row-major, 1 = the column is
 * left out for that row).  In f32 throughout:
 *
 *   E_c  = LN_tok(tok_last[cand[c]])                     (g_mlp_layernorm, eps 1e-12)
 *   s_bc = (u_b / max(|u_b|, 1e-8)) . (E_c / max(|E_c|, 1e-8))   (F.cosine_similarity)
 *   z_bc = s_bc * inv_tau;  cand[c] < 0 or mask[b][c] -> -inf
 *   loss = mean_b (logsumexp_c z_bc - z_b,target[b])     (CrossEntropyLoss, mean)
 *
 * The sampled form -- cand = the row-major [B, 1 + K] block of news_ind_pos_neg
 * (data_utils.py:275-334, 512-578, 794-817), target[b] = b (1 + K), mask = every
 * column outside row b's block, inv_tau = 1 -- is the reference's commented loss
 * (trainer.py:612-625: cosine logits [B, 1 + K], pads set to -inf,
 * CrossEntropyLoss() against column 0).  The in-batch form keeps every column but
 * the pads and the row's other clicked news.
 *
 * Every sum has a fixed order (no float atomics): two runs of one batch give the
 * same bits.  The entries read target, cand and mask back to the host (one
 * synchronising copy) and refuse, before any launch, a target[b] outside [0, Cn)
 * or on a column that is a pad or masked for row b (NR_ERR_INVALID).
 */
#ifndef NEWSREC_CONTRASTIVE_H
#define NEWSREC_CONTRASTIVE_H

#include "newsrec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The stand-alone stage over an f32 table E [U][lde] (lde >= 1024, % 4 == 0), the
 * sibling of nr_cosine_margin (trainer.py:612-625).  Written: *loss, du [B][1024],
 * dE_cols [Cn][1024] (the gradient of E[cand[c]] PER COLUMN, zero rows for pads:
 * not scattered into a [U] table), logits_out (nullable, [B][Cn]: z with its
 * -inf entries).  ws: nr_cosine_infonce_workspace_bytes, 256-byte aligned.
 * The call has no row count of E: every cand[c] >= 0 must be a row of E (as pos / neg of
 * nr_cosine_margin), it is NOT range-checked and a larger index reads out of bounds on the
 * device.  (The train-step entries know U and refuse cand[c] >= U.) */
int64_t nr_cosine_infonce_workspace_bytes(int64_t B, int64_t Cn);
int nr_cosine_infonce(int64_t B, int64_t Cn, const float* users, const float* E, int64_t lde, const int32_t* cand,
                      const int32_t* target, const uint8_t* mask, float inv_tau, float* logits_out, float* loss,
                      float* du, float* dE_cols, void* ws, int64_t ws_bytes, void* stream);

/* The loss of a contrastive train step (device pointers; mask nullable). */
typedef struct nr_contrastive_spec {
  int64_t Cn;
  const int32_t* cand;   /* [Cn] */
  const int32_t* target; /* [B] */
  const uint8_t* mask;   /* nullable [B][Cn] */
  float inv_tau;
} nr_contrastive_spec;

/* nr_final_train_step (trainer.py:1044-1066) with the loss above in place of the
 * margin loss (trainer.py:612-625 instead of :1058-1066): same arguments, outputs
 * and workspace contract; args->pos, neg and margin are ignored. */
int64_t nr_final_train_step_contrastive_workspace_bytes(int dtype, int64_t B, int64_t U, int64_t Hs, int64_t Cn);
int nr_final_train_step_contrastive(const nr_final_train_args* args, const nr_contrastive_spec* spec, void* ws,
                                    int64_t ws_bytes, void* stream);

/* nr_latent_train_step with the same loss (trainer.py:612-625 over the latent pooler's
 * normalized users): same arguments, outputs and workspace contract; args->pos, neg and
 * margin are ignored. */
int64_t nr_latent_train_step_contrastive_workspace_bytes(int dtype, int64_t B, int64_t U, int64_t Hs, int64_t Cn);
int nr_latent_train_step_contrastive(const nr_latent_train_args* args, const nr_contrastive_spec* spec, void* ws,
                                     int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NEWSREC_CONTRASTIVE_H */
