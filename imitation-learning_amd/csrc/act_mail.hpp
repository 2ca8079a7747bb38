// The acting worker's device protocol (include/il_hip.h il_act_step: the contract; this header: the one place on the device side that knows the layout). Shared by
// k_act_step / k_act_step_population (sac.hip), k_act_step_general / k_act_commit_general (general.hip) and k_pwil_couple (pwil.hip); at the end, the mailbox of the lockstep
// evaluation launch (k_act_eval_rows, sac.hip).
#pragma once
#include "il_common.hpp"

// ---- mailbox (pinned host memory): IL_MAIL_HEADER words, then next_state | observation | action | echo, the vectors padded to 4 floats ----
enum { ACT_MAIL_COMMIT = 0, ACT_MAIL_REWARD = 2, ACT_MAIL_TERMINAL = 3, ACT_MAIL_TIMEOUT = 4, ACT_MAIL_STEP = 5,   // ([TERMINAL + 1] is TIMEOUT, like the two ring columns)
       ACT_MAIL_NOISE_OFFSET = 6 };   // il_act_step_population: this learner's Philox offset as raw uint32 bits, written before the commit word (the one-learner entry points take it as an argument)
template <class F>
struct ActMail {
  F* mail; int o_next, o_obs, o_act, o_echo;
  int ld;   // the observation as a one-row matrix: its padded length
  __host__ __device__ F* next() const { return mail + o_next; }   // next_state of the pending transition
  __host__ __device__ F* obs() const { return mail + o_obs; }     // observation to act on
  __host__ __device__ F* act() const { return mail + o_act; }     // action (device -> host; written back by the host under IL_ACT_CARRY_FROM_MAILBOX)
  __host__ __device__ F* echo() const { return mail + o_echo; }   // echo of the commit word
  __host__ __device__ int floats() const { return (o_echo + 1 + 15) & ~15; }   // il_act_mailbox_floats
};
template <class F>
__host__ __device__ inline ActMail<F> act_mail(F* mail, int S, int A) {
  const int Sp = (S + 3) & ~3, Ap = (A + 3) & ~3;
  return ActMail<F>{mail, IL_MAIL_HEADER, IL_MAIL_HEADER + Sp, IL_MAIL_HEADER + 2 * Sp, IL_MAIL_HEADER + 2 * Sp + Ap, Sp};
}

// ---- carry (device, S + A + 4 floats): state | action of the pending transition, then three words ----
__host__ __device__ inline int act_carry_consumed(int S, int A) { return S + A; }      // commit word of the last appended transition
__host__ __device__ inline int act_carry_reward(int S, int A) { return S + A + 1; }    // IL_ACT_REWARD_ON_DEVICE: the reward il_pwil_act_reward computed ...
__host__ __device__ inline int act_carry_coupled(int S, int A) { return S + A + 2; }   // ... and the commit word of the post it computed it for

// a transition is posted and no launch has appended it yet: carry remembers the commit word of the last appended one, so a launch that runs again without a new post
// (a replayed graph, or a launch still queued when the host posts the next step) appends - and couples - each transition exactly once
__device__ __forceinline__ bool act_pending(unsigned word, const float* carry, int S, int A) {
  return (word & IL_ACT_PENDING) && __float_as_uint(carry[act_carry_consumed(S, A)]) != word;
}

struct ActPost {
  ActMail<float> m; float commit; unsigned word, flags; bool pending, wrap, uncoupled; long long cursor, cap;
};
// what this launch has to do: the commit word (sequence << 6 | IL_ACT_* flags, the LAST thing the host writes: one 4-byte store publishes the post), whether its
// transition is still to be appended, and the cursor - every thread reads them here, before anything below is written
__device__ __forceinline__ ActPost act_post(float* mail, const float* carry, const long long* ring_state, int S, int A) {
  ActPost p;
  p.m = act_mail(mail, S, A);
  p.commit = mail[ACT_MAIL_COMMIT];
  p.word = (unsigned)p.commit; p.flags = p.word & 63u;
  p.cursor = ring_state[0]; p.cap = ring_state[2];
  p.pending = act_pending(p.word, carry, S, A);
  p.wrap = p.pending && (p.flags & IL_ACT_WRAP_ABSORBING);
  // a reward computed on the device belongs to the post whose commit word il_pwil_act_reward left in the coupled slot: a pending post it has not coupled (a replayed launch
  // overtaken by the host's next post) is left alone - no row, no action, no echo (the caller returns, block-uniform) - for the coupling + append pair the host enqueues
  // behind that post
  p.uncoupled = p.pending && (p.flags & IL_ACT_REWARD_ON_DEVICE) && __float_as_uint(carry[act_carry_coupled(S, A)]) != p.word;
  return p;
}
// memory.py:40-44 append (+ memory.py:65-68 absorbing wrap) of the pending transition into ring row(s) of `row` floats: one column per thread per trip
__device__ __forceinline__ void act_append(const ActPost& p, const float* carry, float* ring, int row, int S, int A) {
  if (!p.pending) return;
  const int o_next = S + A, o_rew = 2 * S + A;
  const float* mail = p.m.mail;
  for (int c = threadIdx.x; c < row; c += blockDim.x) {
    float v = 0.f;
    if (c < o_next) v = (p.flags & IL_ACT_CARRY_FROM_MAILBOX) ? (c < S ? p.m.obs()[c] : p.m.act()[c - S]) : carry[c];   // state | action of the transition
    else if (c < o_rew) v = p.wrap ? (c == o_rew - 1 ? 1.f : 0.f) : p.m.next()[c - o_next];   // next_state, or the absorbing state (memory.py:67)
    else if (c == o_rew) v = (p.flags & IL_ACT_REWARD_ON_DEVICE) ? carry[act_carry_reward(S, A)] : mail[ACT_MAIL_REWARD];   // reward (posted, or left by il_pwil_act_reward ahead of this launch)
    else if (c == o_rew + 1) v = p.wrap ? 0.f : mail[ACT_MAIL_TERMINAL];                      // terminal (cleared by the wrap)
    else if (c == o_rew + 2) v = mail[ACT_MAIL_TIMEOUT];                                      // timeout
    else if (c == o_rew + 3) v = 1.f;                                                         // weight
    else if (c == o_rew + 4) v = mail[ACT_MAIL_STEP];                                         // step
    ring[p.cursor * row + c] = v;
    if (p.wrap) {  // absorbing -> absorbing row (memory.py:68)
      float w = 0.f;
      if (c < S) w = (c == S - 1) ? 1.f : 0.f;
      else if (c >= o_next && c < o_rew) w = (c == o_rew - 1) ? 1.f : 0.f;
      else if (c == o_rew + 3) w = 1.f;
      else if (c == o_rew + 4) w = mail[ACT_MAIL_STEP];
      ring[((p.cursor + 1) % p.cap) * row + c] = w;
    }
  }
}
// the cursor, the `full` flag and the consumed commit word move only here, by one thread behind the launch's LAST barrier: an append-only launch (IL_ACT_NO_ACTION) has no
// other barrier between the waves' loads of ring_state[0] / the consumed word in act_post and these stores, and with rows wider than one wave (Ant: 240 floats) a wave that
// loaded late would have written its columns into the next row (the race the host emulation found). Then the echo, stored last with system-scope release.
__device__ __forceinline__ void act_commit(const ActPost& p, float* carry, long long* ring_state, int S, int A) {
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    if (p.pending) {
      const long long adv = p.wrap ? 2 : 1, nc = p.cursor + adv;
      ring_state[0] = nc % p.cap;
      if (nc >= p.cap) ring_state[1] = 1;
      carry[act_carry_consumed(S, A)] = __uint_as_float(p.word);
    }
    __hip_atomic_store(p.m.echo(), p.commit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- lockstep evaluation mailbox (il_act_eval_rows; pinned host memory): IL_MAIL_HEADER words, then observations [max_rows][Sp] | actions [max_rows][Ap] | one echo word per
// 16-row tile, Sp / Ap = S / A rounded up to 4 floats, the total to 16. Host -> device: the observation rows, the row count, then the commit word (sequence * 64 + flags, the
// LAST thing the host writes); device -> host: the action rows [0, n) and every tile's echo of the commit word. No next_state, no carry: the launch changes nothing on the device.
enum { EVAL_MAIL_COMMIT = 0, EVAL_MAIL_ROWS = 1 };   // [1]: n, the rows in use this step (as a float: 0 <= n <= max_rows <= 1024)
template <class F>
struct EvalMail {
  F* mail; int o_obs, o_act, o_echo, ld_obs, ld_act, tiles;
  __host__ __device__ F* obs() const { return mail + o_obs; }     // row r: obs() + r * ld_obs
  __host__ __device__ F* act() const { return mail + o_act; }     // row r: act() + r * ld_act
  __host__ __device__ F* echo() const { return mail + o_echo; }   // tile t: echo()[t]
  __host__ __device__ int floats() const { return (o_echo + tiles + 15) & ~15; }   // il_eval_mailbox_floats
};
template <class F>
__host__ __device__ inline EvalMail<F> eval_mail(F* mail, int S, int A, int max_rows) {
  const int Sp = (S + 3) & ~3, Ap = (A + 3) & ~3;
  return EvalMail<F>{mail, IL_MAIL_HEADER, IL_MAIL_HEADER + max_rows * Sp, IL_MAIL_HEADER + max_rows * (Sp + Ap), Sp, Ap, (max_rows + 15) / 16};
}
