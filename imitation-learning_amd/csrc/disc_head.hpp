// What the four adversarial discriminators (gail.hip, gail_shaped.hip, gail_deep.hip, gail_shaped_deep.hip) do with the logit once their networks have produced
// it: the calls of an update, the loss head dL/dz (reference training.py:97-113) and the reward head (models.py:177-180). The networks differ; this part does not, and
// it lives here once. The descriptor structs (il_disc, il_disc_shaped, il_disc_deep, il_disc_shaped_deep) name every field the head reads the same way, so the
// functions that read them are templates on the descriptor type. Each call site keeps what differs: where f, w and the mix draw live in LDS, which threads own a row,
// and what is done with dz. Every function keeps the operations and their order of the copies it replaces: results are bit-identical.
#pragma once
#include "il_common.hpp"

// Calls of one update: BCE and PUGAIL run {policy, expert}, Mixup ONE call on the convex combinations (training.py:104-113); plus the gradient-penalty mix (:116-126)
template <class Desc>
__host__ __device__ inline int disc_calls(const Desc& d) { return (d.loss_function == IL_LOSS_MIXUP ? 1 : 2) + (d.grad_penalty > 0.f ? 1 : 0); }
// what a call runs on: 0 policy, 1 expert, 2 gradient-penalty mix, 3 Mixup mix
template <class Desc>
__host__ __device__ inline int disc_kind(const Desc& d, int call) { return d.loss_function == IL_LOSS_MIXUP ? (call == 0 ? 3 : 2) : call; }
// log pi(a|s) of subtract_log_policy for the rows of a first-order call (models.py:175: z = f - log pi, a pure shift), or nullptr
// (the three pointers, not the struct: a reference to gail.hip's globalized copy of it changed k_gail_grad's instructions)
__device__ __forceinline__ const float* disc_logit_offset(const float* policy, const float* expert, const float* mix, int kind) {
  return kind == 0 ? policy : (kind == 1 ? expert : (kind == 3 ? mix : nullptr));
}

// PUGAIL with a finite nonnegative_margin (training.py:100-102): a value pass leaves the per-tile sums of w softplus(z) = w bce(z, 0) of the policy call in ws[pu + [0, nt)] and
// of the expert call in ws[pu + [nt, 2 nt)]; the gradient pass sums them in tile order - every workgroup the same way - and decides whether torch.clamp(min = -margin) passes the
// gradient (1) or not (0). With nonnegative_margin = inf (pu_clamped = 0) and for the other losses it always does.
template <int R>
__device__ __forceinline__ float disc_tile_sum(float v) {   // the first R lanes of a wave (R = 16 or 32, all of them active): sum of their values in lane order
  float part = 0.f;
  for (int o = 0; o < R; ++o) part += __shfl(v, o, R);
  return part;
}
template <class Desc>
__device__ __forceinline__ float disc_pu_gate(const Desc& d, const float* ws, int64_t pu, int nt, float fB) {
  if (d.loss_function != IL_LOSS_PUGAIL || !d.pu_clamped) return 1.f;   // (no value pass ran: nothing to read)
  float se = 0.f, sp = 0.f;
  for (int t = 0; t < nt; ++t) { sp += ws[pu + t]; se += ws[pu + nt + t]; }
  return d.pos_class_prior * (se / fB) - sp / fB >= -d.nonnegative_margin ? 1.f : 0.f;   // gradient where the input is not below the bound
}

// d loss / d z of one row = w (c_sig sigmoid(z) - c_lab) / B (+ the entropy bonus): BCE {1, label}; PUGAIL policy {-1, 0}, expert {2 prior, prior} (clamped away:
// policy {0, 0}, expert {prior, prior}); Mixup {1, the row's draw `mix`}
template <class Desc>
__device__ __forceinline__ float disc_dz(const Desc& d, float z, float w, int kind, float pu_on, float mix, float fB) {
  const bool pu = d.loss_function == IL_LOSS_PUGAIL;
  const float c_sig = pu ? (kind == 1 ? (1.f + pu_on) * d.pos_class_prior : -pu_on) : 1.f;
  const float c_lab = kind == 3 ? mix : (kind == 1 ? (pu ? d.pos_class_prior : 1.f) : 0.f);
  const float p = sigmoid_f(z);
  float dz = w * (c_sig * p - c_lab) / fB;
  if (d.entropy_bonus > 0.f) dz += d.entropy_bonus * w * z * p * (1.f - p) / fB;
  return dz;
}

// AIRL (0) / GAIL (1) / FAIRL (2) reward of the logit z (models.py:177-180)
__device__ __forceinline__ float disc_reward_head(int reward_function, float z) {
  const float Dp = sigmoid_f(z);
  float h = reward_function == 1 ? -log1pf(-Dp + 1e-6f) : logf(Dp + 1e-6f) - log1pf(-Dp + 1e-6f);
  if (reward_function == 2) h = expf(h) * -h;
  return h;
}
