/*
 * fenv.h -- C ABI of the MI355X (gfx950) batched formation env + policy rollout library
 * (libfenv.so, built from marl-distributedformation_amd/csrc/).
 *
 * The reference exposes this hot path as the stable-baselines3 VecEnv Python object
 * FormationEnv (/root/reference/vectorized_env.py:16-109) over per-formation
 * FormationSimulator objects (/root/reference/simulate.py:7-254), plus SB3's MlpPolicy
 * forward (call site vectorized_env.py:126).  Each entry point below replaces one piece of that
 * interface; the Python mirror (marl-distributedformation_amd/vectorized_env.py) keeps the
 * reference's method names and binds these symbols with ctypes.
 *
 * Conventions
 *  - Plain C types only.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - Every buffer argument named obs/act/rew/done/out/params/... is a DEVICE pointer owned
 *    by the caller unless the name ends in `_host`.  Env state is owned by the handle.
 *  - Layouts: act [T][A][2] f32, obs [T][A][D] f32 (D = 8 if goal_in_obs else 6),
 *    rew [T][A] f32, done [T][A] u8 (0/1), with A = num_formation * num_agents and agents of
 *    formation f at rows f*N .. f*N+N-1 (vectorized_env.py:72-79 ordering).
 *  - All calls are asynchronous on `stream` unless stated; none throws.  Return 0 on success,
 *    a negative FENV_E* code on failure; fenv_last_error() gives a thread-local message.
 *  - One handle is used from one host thread at a time.
 */
#ifndef FENV_H
#define FENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  A host program compiled against one revision checks
 * fenv_abi_version() == FENV_ABI_VERSION at start-up: a signature that changed between revisions
 * gets a new symbol name, never a reordered argument list under the old one.
 *   1  round-1/2 entry points (policy_forward with row0)
 *   2  + fenv_abi_version, fenv_get_state_range, fenv_metrics_range, ppo_workspace_bytes,
 *        ppo_update_ws, ppo_grad, ppo_apply, fenv_test_ppo_inject
 *   3  + fenv_status, fenv_test_stage_hook, fenv_pinned_pool_bytes, fenv_debug_staging (no
 *        signature changed)
 *   4  + fenv_host_alloc, fenv_host_free (no signature changed)
 *   5  + fenv_stream_gate (no signature changed)
 *   6  + fenv_control, fenv_rollout_velocity, fenv_rollout_control, fenv_control_neighbor_dist
 *        (no signature changed) */
#define FENV_ABI_VERSION 6
int fenv_abi_version(void);

typedef struct fenv fenv_t;

enum {
    FENV_OK = 0,
    FENV_EINVAL = -1,  /* bad argument (shape/size/pointer/mode) */
    FENV_EHIP = -2,    /* HIP runtime error (no device, launch failure, ...) */
    FENV_ESTATE = -3,  /* operation not valid in the handle's current state */
    FENV_ENOMEM = -4
};

/* Reset RNG modes. */
enum {
    /* Bit-for-bit the reference: one global MT19937 stream seeded like torch.manual_seed(seed),
       drawn on the host in formation order (simulate.py:125,133,140) and staged to HBM. */
    FENV_RESET_MT19937 = 0,
    /* Throughput mode: counter-based Philox4x32-10 keyed by (seed, global formation, episode),
       drawn inside the kernels.  Same distributions, not the reference's stream. */
    FENV_RESET_PHILOX = 1
};

/* Replaces FormationEnv.__init__ (vectorized_env.py:22-50) for the formations
 * [first_formation, first_formation + num_formation) of a batch of total_formations
 * (sharding; pass 0 and num_formation for an unsharded env).  Like the reference ctor it
 * consumes the first reset draw set (simulate.py:61).  share_reward_ratio is the simulator's
 * (simulate.py:11; the reference env never forwards its cfg key, so pass 0.25 for parity).
 * Formation sizes: 1 <= num_agents <= FENV_MAX_AGENTS (the reference takes any size; up to 64
 * agents a wavefront holds whole formations, up to 1024 a workgroup holds one formation, larger
 * formations run several agents per thread with the exchanges through global scratch). */
#define FENV_MAX_AGENTS (1 << 24)
int fenv_create(fenv_t **out, int32_t device, int64_t num_formation, int32_t num_agents,
                int32_t goal_in_obs, double share_reward_ratio, int32_t max_steps, uint32_t seed,
                int32_t reset_mode, int64_t first_formation, int64_t total_formations);

/* Frees the handle and every device/pinned buffer it owns.  Safe at any point: it restores the
 * caller's current device, waits for the handle's own staging copy (hipFree then waits for the
 * device's work), and a free that the runtime refuses because a stream capture is under way is
 * parked and retried by the next fenv_create / fenv_destroy.  The library keeps the set of live
 * handles: a pointer not in it (a second destroy, or never created) returns FENV_EINVAL without
 * its memory being read. */
int fenv_destroy(fenv_t *env);

/* FENV_RESET_MT19937 staging check.  Every staged reset set carries per-draw tags (computed from
 * the draws' bits, their index and the set's generation); the kernels verify them when they apply
 * a reset, and a failure is recorded in the handle.  From then on every call on the handle
 * (fenv_reset, fenv_observe, fenv_step, fenv_rollout*, fenv_policy_rollout, fenv_metrics*,
 * fenv_get_state*, fenv_set_state, fenv_status) returns FENV_ESTATE with a message naming the
 * generation, the formation and whether the set read was the slot's previous one, the other
 * slot's, or neither.  A failure is seen by the first call after the failing launch has run:
 * fenv_status after a synchronize of the launch stream reports it (host read, no GPU call). */
int fenv_status(const fenv_t *env);

/* Test hooks of the MT19937 staging (host only).  The next n_refills staging copies, of any
 * handle, run in `mode`: 1 = the copy (a DMA on the handle's staging stream) starts ~0.35 ms
 * late, behind a sleeping kernel (a launch that were not ordered behind its refill would read the
 * slot's old set); 2 = the copy is skipped (the slot keeps its old set: the tag check must fire).
 * mode 0 / n_refills 0 turns the hook off. */
void fenv_test_stage_hook(int32_t mode, int32_t n_refills);

/* Bytes of pinned staging buffers cached for reuse on `device` (bounded at 512 MiB per device;
 * a destroyed env's buffer is freed instead when the pool is full). */
int64_t fenv_pinned_pool_bytes(int32_t device);

/* Host memory the kernels read and write in place (zero-copy): coherent host memory mapped into
 * the device's address space, *dev its device address.  The host faces of reset / step
 * (FormationEnv.reset / step with numpy arrays, vectorized_env.py:52-55, 68-82) pass the `dev`
 * addresses of such a block as act / obs / rew / done to fenv_reset / fenv_step and synchronize the
 * stream: no DMA copies (config 0, 1,000 x 5: 20.7 us per step against 58.2 us through pinned
 * mirrors and four hipMemcpyAsync).  Blocks come from the same pooled, bounded pinned cache as the
 * MT19937 staging sets; `bytes` is rounded up to 256. */
int fenv_host_alloc(int32_t device, int64_t bytes, void **host, void **dev);
/* Returns a fenv_host_alloc block (host address) to `device`'s pool; NULL is a no-op.  The caller
 * makes sure no queued launch still reads or writes it. */
int fenv_host_free(int32_t device, void *host);

/* Diagnostic (synchronous): info_host[0..9] = {slot the next reset reads, generation of slot 0,
 * of slot 1, floats per staged set, error words 0..2, next generation, device address of the
 * terminal-state records, of the staged sets}; with out_host (floats per
 * staged set) the staged set of device slot `which` (0, 1) or of host slot which - 2 (2, 3);
 * which = 4: the terminal-state records (px, py, gx, gy)[A] (4 A floats; any reset mode). */
int fenv_debug_staging(fenv_t *env, int32_t which, float *out_host, int64_t *info_host);

/* out_host[0..7] = {num_formation, num_agents, obs_dim, num_agents_total(A), steps_since_reset
 * (common value, -1 if formations differ), reset_mode, first_formation, total_formations}. */
int fenv_info(const fenv_t *env, int64_t *out_host);

/* Replaces FormationEnv.reset (vectorized_env.py:52-55): new draw set for every formation, then
 * compute_observations (:57-66) into obs [A][D] (obs may be NULL). */
int fenv_reset(fenv_t *env, float *obs, void *stream);

/* compute_observations (vectorized_env.py:57-66 / simulate.py:150-174) of the current state. */
int fenv_observe(fenv_t *env, float *obs, void *stream);

/* Replaces FormationEnv.step (vectorized_env.py:68-82) -> FormationSimulator.step
 * (simulate.py:70-118) for every formation: act [A][2] in the SB3 action space (the env scales
 * by 10 and does not clip, vectorized_env.py:69-70), obs [A][D] post-auto-reset, rew [A],
 * done [A].  rew/done/obs may be NULL to skip writing them. */
int fenv_step(fenv_t *env, const float *act, float *obs, float *rew, uint8_t *done,
              void *stream);

/* T consecutive env.step calls fused in one launch (state kept on chip): act [T][A][2],
 * obs [T][A][D] (obs[k] = observation returned by step k), rew [T][A], done [T][A].
 * Bit-identical to T fenv_step calls.  partial (may be NULL) receives one {sum reward,
 * sum done} float pair per group of 4 wavefronts (N <= 64) or per formation (N > 64) --
 * fenv_partial_count of them, overwritten by every launch -- for fenv_reduce_partials. */
int fenv_rollout(fenv_t *env, int32_t T, const float *act, float *obs, float *rew,
                 uint8_t *done, float *partial, void *stream);

/* Synthetic random-action rollout ("act_seed | act"; the north star's
 * "synthetic random-action rollouts"): as fenv_rollout, but the actions are drawn inside the
 * kernel instead of read from HBM.  Component c of agent a's action at step k is
 * (w >> 8) / 2^23 - 1, exactly, in [-1, 1), with w = word (2 (s & 1) + c) of
 * Philox4x32-10(counter = (g, s >> 1), key = act_seed), s = step_offset + k the global step
 * index and g = the global agent index (first_formation * N + a: shard-invariant).  act_out
 * (may be NULL) receives the actions [T][A][2]; feeding them to fenv_rollout from the same state
 * gives bit-identical results. */
int fenv_rollout_random(fenv_t *env, int32_t T, uint64_t act_seed, uint64_t step_offset,
                        float *act_out, float *obs, float *rew, uint8_t *done, float *partial,
                        void *stream);

/* ------------------------------------------------------------------ baseline controller
 * The reference's potential-field formation controller control(i, env) (simulate.py:256-319, run
 * by `python simulate.py`, :321-329): the baseline the RL policy is compared with.  It steps a
 * FormationSimulator with a raw velocity (simulate.py:70 step(input_velocity)); the x10 action
 * scaling belongs to FormationEnv.step one layer up (vectorized_env.py:69-70), and
 * 10 * (v / 10) is not v in fp32, so fenv_step / fenv_rollout cannot carry a controller's
 * velocity bit-exactly: the velocity entry points below can.  All three take formations of at
 * most 1,024 agents (FENV_EINVAL above: the large-formation path has no controller kernels).
 *
 * fenv_control: the velocity control() hands to env.step for every agent of the current state,
 * vel [A][2] (simulate.py:262-319 in the reference's fp32 operation order: spring terms towards
 * the next, previous and opposite agents with rest lengths pi * 40 / N, pi * 40 / N and 80,
 * clipped to [-1, 1] per component, plus the clipped goal attraction; coincident agents give
 * NaN as in the reference).  The state is not changed.  num_agents must be even
 * (simulate.py:279 asserts it): FENV_EINVAL otherwise. */
int fenv_control(fenv_t *env, float *vel, void *stream);

/* FormationSimulator.step(input_velocity) (simulate.py:70-118) of every formation, T times in
 * one launch: vel [T][A][2] is added to the positions unscaled (simulate.py:82).  Everything else
 * -- obs / rew / done layouts, NULL outputs, the partial records and fenv_partial_count, the
 * split at MT19937 reset events -- is fenv_rollout's.  Any 1 <= num_agents <= 1024. */
int fenv_rollout_velocity(fenv_t *env, int32_t T, const float *vel, float *obs, float *rew,
                          uint8_t *done, float *partial, void *stream);

/* T steps of control(i, env) for every formation fused in one launch (the reference's animation
 * loop, simulate.py:324-328): per step the controller's velocities are computed from the state
 * held on chip and applied as fenv_rollout_velocity applies them.  vel_out (may be NULL)
 * receives them, [T][A][2].  Bit-identical to T x (fenv_control + fenv_rollout_velocity(T = 1)).
 * num_agents must be even. */
int fenv_rollout_control(fenv_t *env, int32_t T, float *vel_out, float *obs, float *rew,
                         uint8_t *done, float *partial, void *stream);

/* Host-only: the controller's fp32 desired neighbour distance, pi * desired_radius / num_agents
 * with desired_radius = 40 (simulate.py:259, :286; not the reward's radius of 60, :25). */
float fenv_control_neighbor_dist(int32_t num_agents);

/* Number of float2 partial records fenv_rollout writes (see fenv_rollout; independent of T). */
int64_t fenv_partial_count(const fenv_t *env);

/* Diagnostic (host only): name of the kernel fenv_rollout launches for a T-step launch of this
 * env (for matching rocprofv3 kernel traces to bench lines). */
const char *fenv_rollout_kernel(const fenv_t *env, int32_t T);

/* Deterministic fixed-order reduction of `count` partial records into out[2] (double, device):
 * {sum of rewards, sum of agent-dones}. */
int fenv_reduce_partials(const float *partial, int64_t count, double *out, void *stream);

/* Launch gate (no reference counterpart: the reference steps one Python loop, vectorized_env.py
 * :71-79).  Enqueues one wavefront on `stream` that holds every later launch on the stream until the
 * 32-bit word at `flag` equals `value`, or until timeout_us (0 < timeout_us <= 60 s) of the device's
 * constant-rate clock have passed -- the wave always exits, so a host that never stores the value
 * costs the stream timeout_us, never a hang.  `flag` is a device address, normally inside a
 * fenv_host_alloc block (the host stores the value with a plain write; the kernel polls it with
 * system-scope loads over the bus).  status (device address, may be NULL; 16 bytes, 8-byte
 * aligned) receives status[0] = 1 (released by the flag) or 2 (timed out), status[1] = the number
 * of polls and status[2..3] = the time the wave held the stream, entry to exit, in ns (uint64,
 * little-endian; from the constant-rate clock), status[0] written last.
 * Use: enqueue a batch of launches behind the gate, then release it, so the host's issue time of
 * the batch is off the device's critical path (bench.py's timed region). */
int fenv_stream_gate(const uint32_t *flag, uint32_t value, int64_t timeout_us, uint32_t *status,
                     void *stream);

/* Per-formation statistics the reference logs to wandb (rew [A] may be NULL -> 0), out [F][8] f32:
 *   0 avg_dist_to_goal, 1 ave_dist_to_neighbor, 2 std_dist_to_neighbor (unbiased, NaN when
 *     N == 1): compute_metrics (simulate.py:238-254) on the current (post-reset) state;
 *   3 mean reward (vectorized_env.py:80-81);
 *   4 close_to_goal_reward, 5 reward_dist, 6 reward_right_neighbor, 7 reward_left_neighbor:
 *     means over the formation's agents of compute_reward_and_done's components
 *     (simulate.py:183-208) for the state the env's latest step scored -- the terminal
 *     (pre-reset) state of a formation that step reset; after fenv_reset / fenv_set_state,
 *     of the current state.
 * Means are summed in agent order in double.  sums (may be NULL) [8] double = column sums over F. */
int fenv_metrics(fenv_t *env, const float *rew, float *out, double *sums, void *stream);

/* State access (device buffers): px,py [A], gx,gy [F], t [F] = steps_since_reset.
 * fenv_set_state synchronises `stream` to read back t; in FENV_RESET_MT19937 mode all t
 * must be equal (the reference keeps formations in lock-step) or FENV_EINVAL is returned. */
int fenv_get_state(fenv_t *env, float *px, float *py, float *gx, float *gy, int32_t *t,
                   void *stream);
int fenv_set_state(fenv_t *env, const float *px, const float *py, const float *gx,
                   const float *gy, const int32_t *t, void *stream);

/* One formation range [first, first + count) of the handle's shard (FormationEnv.formationsim_list
 * [i], vectorized_env.py:38-43 / simulate.py:133-147): fenv_get_state's buffers for those
 * formations only -- px,py [count*N], gx,gy,t [count] -- so a view costs O(count*N), not O(A). */
int fenv_get_state_range(fenv_t *env, int64_t first, int64_t count, float *px, float *py,
                         float *gx, float *gy, int32_t *t, void *stream);
/* fenv_metrics over formations [first, first + count) only: rew [count*N] (may be NULL),
 * out [count][8], sums [8] (may be NULL).  Values equal the matching rows of fenv_metrics. */
int fenv_metrics_range(fenv_t *env, int64_t first, int64_t count, const float *rew, float *out,
                       double *sums, void *stream);

/* Host-only (no GPU needed): the reset positions the reference's global MT19937 stream gives
 * formations [first, first+count) of a draw set of `total` formations that starts `skip_sets`
 * draw sets after torch.manual_seed(seed).  px,py [count*N], gx,gy [count] host buffers. */
int fenv_host_reset_draws(uint32_t seed, int64_t skip_sets, int64_t total, int64_t first,
                          int64_t count, int32_t num_agents, float *px_host, float *py_host,
                          float *gx_host, float *gy_host);

/* Diagnostic: one of the kernels' fp32 primitives over n device inputs (op 0: a/400,
 * 1: a/600, 2: sqrtf(a), 3: sqrtf(fmaf(b, b, a*a))) into out; for parity tests. */
int fenv_fp_probe(int32_t op, const float *a, const float *b, float *out, int64_t n, void *stream);

/* Host-only: the fp32 desired neighbour distance the reference uses (simulate.py:26). */
float fenv_desired_neighbor_dist(int32_t num_agents);

/* ------------------------------------------------------------------ policy (SB3 MlpPolicy)
 * Actor-critic MLP forward as SB3's ActorCriticPolicy with default net_arch for a Box action
 * space: pi: D->64->64 (tanh) -> mu[2]; vf: D->64->64 (tanh) -> value; action =
 * mu + exp(log_std) * eps, log_prob = sum_j Normal(mu_j, exp(log_std_j)).log_prob(action_j),
 * clipped = clamp(action, -1, 1) (what collect_rollouts hands to env.step).
 *
 * params: flat f32 buffer (device), SB3 state_dict order (policy_param_count floats):
 *   pi0.W[64][D] pi0.b[64] pi2.W[64][64] pi2.b[64] vf0.W[64][D] vf0.b[64] vf2.W[64][64]
 *   vf2.b[64] act.W[2][64] act.b[2] val.W[1][64] val.b[1] log_std[2]
 * obs [B][D]; outputs (each may be NULL): mu [B][2], value [B], action [B][2] (unclipped
 * sample, or mu if deterministic), logp [B], clipped [B][2].  eps ~ N(0,1) from Philox keyed
 * by seed with counter (row0 + row, offset): pass row0 = the global index of row 0 (a shard's
 * first agent) so that sharded and unsharded batches draw the same noise per agent. */
int policy_param_count(int32_t obs_dim);
int policy_forward(const float *params, int32_t obs_dim, const float *obs, int64_t B,
                   int64_t row0, float *mu, float *value, float *action, float *logp,
                   float *clipped, uint64_t seed, uint64_t offset, int32_t deterministic,
                   void *stream);

/* SB3 RolloutBuffer.compute_returns_and_advantage (GAE) over [T][A] device buffers:
 * rew, values f32, episode_starts u8 (1 where step k began an episode), last_values [A] f32
 * (value of the observation after the last step), last_dones [A] u8.  Writes advantages and
 * returns (= advantages + values), [T][A] f32. */
int rollout_gae(const float *rew, const float *values, const uint8_t *episode_starts,
                const float *last_values, const uint8_t *last_dones, int32_t T, int64_t A,
                float gamma, float gae_lambda, float *advantages, float *returns, void *stream);

/* ------------------------------------------------------------------ fused PPO rollout
 * Device buffers of one rollout (SB3 RolloutBuffer fields, vectorized_env.py:126-134 n_steps=T).
 * Required: obs, action, value, log_prob, reward, episode_start, last_done.  Optional (NULL to
 * skip): last_obs, mu, clipped, done, last_value, and advantage+ret (both or neither). */
typedef struct fenv_rollout_bufs {
    float *obs;             /* [T][A][D] observation each action was taken on */
    float *last_obs;        /* [A][D] observation after the last step (SB3 _last_obs) */
    float *mu;              /* [T][A][2] policy mean */
    float *action;          /* [T][A][2] unclipped sampled action (what SB3 stores) */
    float *clipped;         /* [T][A][2] clamp(action, -1, 1): what the env was stepped with */
    float *value;           /* [T][A] critic value of obs */
    float *log_prob;        /* [T][A] */
    float *reward;          /* [T][A] */
    uint8_t *episode_start; /* [T][A] 1 where the step began an episode (previous step's done) */
    uint8_t *done;          /* [T][A] */
    uint8_t *last_done;     /* [A] in: episode_start of step 0; out: done of the last step */
    float *last_value;      /* [A] value of last_obs */
    float *advantage;       /* [T][A] GAE(lambda) advantages */
    float *ret;             /* [T][A] advantage + value */
} fenv_rollout_bufs;

/* SB3 collect_rollouts + compute_returns_and_advantage: T steps of every agent in ONE kernel
 * launch -- per step the policy forward (as policy_forward with seed and counter offset+k) and
 * the env step with the clipped action (as fenv_step), then the value of the final observation
 * -- followed by one GAE launch (as rollout_gae) when advantage/ret are given.  Observation 0 is the env's
 * current observation.  The noise of agent a is keyed by its global index (first_formation * N
 * + a), as policy_forward with row0 = first_formation * N, so shards of one batch draw what the
 * unsharded batch draws.  Results are bit-identical to the unfused calls.  Formation sizes
 * 1 <= N <= 64 (larger formations: policy_forward + fenv_step).  In FENV_RESET_MT19937 mode a
 * launch may contain at most one reset event (T <= max_steps + 2). */
int fenv_policy_rollout(fenv_t *env, const float *params, int32_t T, uint64_t seed,
                        uint64_t offset, int32_t deterministic, float gamma, float gae_lambda,
                        const fenv_rollout_bufs *bufs, void *stream);

/* ------------------------------------------------------------------ PPO update
 * SB3 2.x PPO.train for small minibatches (batch_size <= 64, the SB3 default under
 * vectorized_env.py:126-131) in ONE launch (the actor and the critic on one workgroup each,
 * exchanging their gradient-norm partials once per minibatch): for each of n_epochs, the n
 * samples in the order perm[epoch][0..n) split into minibatches of batch_size (the last one
 * partial); per minibatch the clipped surrogate + vf_coef * MSE(returns, values) + ent_coef *
 * entropy loss (advantages normalised per minibatch when normalize_advantage), backward,
 * clip_grad_norm_(max_grad_norm), Adam (torch semantics, bias-corrected).  params [P] (the
 * policy_forward layout) are updated in place; exp_avg / exp_avg_sq [P] and *step (one float)
 * are the Adam state (device); stats (device, 4 doubles) are INCREMENTED by the per-minibatch
 * policy loss, value loss, entropy loss and clip fraction.  Sample buffers (device): obs [n][D],
 * actions [n][2] (unclipped), old_log_prob, advantages, returns [n]; perm int64 [n_epochs][n].
 * If the two workgroups' exchange times out (a workgroup never became resident), the update
 * leaves NaN parameters and marks stats: stats[0] NaN and stats[3] below -1e29. */
typedef struct ppo_hparams {
    float clip_range, ent_coef, vf_coef, max_grad_norm, lr, beta1, beta2, eps;
    int32_t normalize_advantage;
} ppo_hparams;
int ppo_update(float *params, float *exp_avg, float *exp_avg_sq, float *step, int32_t obs_dim,
               const float *obs, const float *actions, const float *old_log_prob,
               const float *advantages, const float *returns, int64_t n, const int64_t *perm,
               int32_t n_epochs, int32_t batch_size, const ppo_hparams *hp, double *stats,
               void *stream);
/* ppo_update with caller-owned exchange words: workspace = ppo_workspace_bytes() of device memory
 * owned by one PPO instance (cleared by each launch on `stream`).  Concurrent updates on
 * different streams must use different workspaces.  (ppo_update itself takes a stream-ordered
 * allocation of its own per launch, hipMallocAsync/hipFreeAsync, so it is safe too.) */
int64_t ppo_workspace_bytes(void);
int ppo_update_ws(float *params, float *exp_avg, float *exp_avg_sq, float *step, int32_t obs_dim,
                  const float *obs, const float *actions, const float *old_log_prob,
                  const float *advantages, const float *returns, int64_t n, const int64_t *perm,
                  int32_t n_epochs, int32_t batch_size, const ppo_hparams *hp, double *stats,
                  void *workspace, void *stream);

/* Data-parallel PPO update ("RCCL ... all-reducing policy gradients"), one
 * global minibatch at a time, each rank holding b_local of its b_global samples:
 *   ppo_grad  -- this rank's share of the minibatch loss gradient on the fused kernel (one
 *                launch, the actor and critic on one CU each): the rows `rows[b_local]` of the
 *                sample buffers (layouts as ppo_update), loss means taken over b_global samples,
 *                advantages normalised with the GLOBAL minibatch's adv_mean / adv_std (when
 *                adv_normalize and b_global > 1), the entropy term included only when
 *                entropy_term (one rank).  grad [P] is overwritten (unclipped); stats [4] are
 *                INCREMENTED by this rank's share of the four loss means (as ppo_update's).
 *                b_local = 0 writes a zero gradient (plus the entropy term if entropy_term).
 *   (the caller all-reduces grad, SUM, over the ranks)
 *   ppo_apply -- clip_grad_norm_(max_grad_norm) + Adam (torch's capturable-Adam operation
 *                order) from the reduced gradient; params / exp_avg / exp_avg_sq / *step as
 *                ppo_update.  Every rank applies the same reduced gradient to the same state. */
int ppo_grad(const float *params, int32_t obs_dim, const float *obs, const float *actions,
             const float *old_log_prob, const float *advantages, const float *returns,
             const int64_t *rows, int32_t b_local, int32_t b_global, float adv_mean,
             float adv_std, int32_t adv_normalize, int32_t entropy_term, const ppo_hparams *hp,
             float *grad, double *stats, void *stream);
int ppo_apply(float *params, float *exp_avg, float *exp_avg_sq, float *step, const float *grad,
              int32_t obs_dim, const ppo_hparams *hp, void *stream);

/* Test hook: the next n_launches fused PPO updates (ppo_update / ppo_update_ws) run as if the two
 * workgroups' norm exchange were lost (the critic never posts; the actor's wait is short), so
 * the NaN-poisoned-update / restore / re-run / raise paths of a caller can be exercised. */
void fenv_test_ppo_inject(int32_t n_launches);

const char *fenv_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* FENV_H */
