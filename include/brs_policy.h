/*
 * brs_policy.h -- C ABI of the on-device rollout side of the path: the caller of the env
 * step in the reference is Stable-Baselines3's PPO with "MlpPolicy" (src/sb_rl.py:63-71) driven by model.learn
 * (src/sb_rl.py:552-556).  Per env step SB3 runs, in Python/torch on the host [3P stable_baselines3]:
 *
 *   brs_policy_act        ActorCriticPolicy.forward(obs): mlp_extractor (separate 6-64-64 tanh towers for pi and vf),
 *                         action_net, value_net, DiagGaussianDistribution.sample() / log_prob(), then the clip of the
 *                         action to the Box before env.step (OnPolicyAlgorithm.collect_rollouts)
 *   brs_rollout_bootstrap collect_rollouts' time-limit handling: rewards[i] += gamma * V(terminal_observation[i]) for
 *                         envs whose episode was truncated, not terminated
 *   brs_gae               RolloutBuffer.compute_returns_and_advantage (GAE(lambda) over the [T][N] buffer)
 *   brs_monitor_update    Monitor / VecMonitor (src/sb_rl.py:501): the return and the length of every episode, summed step
 *                         by step and closed when the env reports terminated or truncated
 *   brs_monitor_reset     evaluate_policy (under EvalCallback, src/sb_rl.py:536-543): with targets, the first target[i]
 *   (with targets)        episodes of env i count and the others are ignored, target[i] = (n_eval_episodes + i) / n
 *   brs_learner_grad      PPO.train(), the body of its minibatch loop: evaluate_actions, the clipped surrogate, the value loss and
 *   brs_learner_apply     the entropy bonus, loss.backward(), clip_grad_norm_, Adam's step, and the target_kl early stop
 *   brs_a2c_grad          A2C.train() (the CLI's `-a A2C`, src/sb_rl.py:72-83 with SB3's defaults): evaluate_actions, -adv log_prob,
 *   brs_a2c_apply         the value loss and the entropy bonus on the whole rollout, clip_grad_norm_, RMSpropTFLike's step
 *
 * and for the reference's second algorithm, DDPG with net_arch = dict(pi=[300, 200], qf=[200, 150]) and
 * NormalActionNoise(sigma=0.1) (src/sb_rl.py:72-83), what SB3's OffPolicyAlgorithm / TD3 do between two gradient steps:
 *
 *   brs_ddpg_act          OffPolicyAlgorithm._sample_action: the deterministic actor (or a uniform action during learning_starts),
 *                         plus the action noise, clipped to the Box
 *   brs_replay_add        ReplayBuffer.add as _store_transition calls it: next_obs is the terminal observation where an episode
 *                         ended, done is cleared where it ended at the time limit only (handle_timeout_termination)
 *   brs_replay_sample     ReplayBuffer.sample: uniform rows and envs, gathered into contiguous minibatch arrays
 *   brs_ddpg_td_target    TD3.train's target with target_policy_noise = 0 and one critic: r + (1 - done) gamma Q'(s', pi'(s'))
 *   brs_ddpg_q            the critic forward Q(s, a)
 *
 * and the gradient step itself (TD3.train as DDPG uses it: one critic, no delay, no target noise):
 *
 *   brs_ddpg_learner_critic_grad  the gradient of mse(Q(s, a), y) w.r.t. the critic
 *   brs_ddpg_learner_actor_grad   the gradient of -mean Q(s, pi(s)) w.r.t. the actor, through the critic to its action inputs
 *   brs_ddpg_learner_apply        torch.optim.Adam's step on one network and polyak_update of its target
 *
 * and TD3's three changes to that recipe (the CLI's `-a TD3`, src/sb_rl.py:73-83, with the DDPG net_arch):
 *
 *   brs_td3_td_target                  TD3.train's target: clipped Gaussian noise on the target action, the minimum of two critics
 *   brs_ddpg_learner_twin_critic_grad  the gradient of mse(Q1(s, a), y) + mse(Q2(s, a), y) w.r.t. both critics in one set of launches
 *                                      (the delay is the caller's: it skips actor_grad and passes target_dev = NULL on the other steps)
 *
 * These entry points do the same arithmetic on the GPU, reading the simulator's outputs in place (device pointers),
 * so that a rollout of 65,536 envs needs no per-env Python and no PCIe traffic.  All buffers are DEVICE pointers owned
 * by the caller; every call only enqueues work on `stream`.  Same library (libbrs_hip.so), same status codes as brs.h.
 *
 * Parameter vector (host floats, brs_policy_set_weights), torch.nn.Linear layout weight[out][in]:
 *   pi: W1[64][6] b1[64] W2[64][64] b2[64] W3[2][64] b3[2]   (mlp_extractor.policy_net.0/.2, action_net)
 *   vf: W1[64][6] b1[64] W2[64][64] b2[64] W3[1][64] b3[1]   (mlp_extractor.value_net.0/.2, value_net)
 *   log_std[2]
 * Noise: z = Box-Muller of Philox4x32-10(counter = (step, 0x504f4c49 "POLI", gid_lo, gid_hi), key = seed), one block per
 * env and step, gid = env_index_base + i: independent of how envs are sharded over GPUs, disjoint from the simulator's
 * streams (whose second counter word is 0).
 */
#ifndef BRS_POLICY_H
#define BRS_POLICY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRS_POLICY_OBS 6
#define BRS_POLICY_HID 64
#define BRS_POLICY_ACT 2
#define BRS_POLICY_NPI (64 * 6 + 64 + 64 * 64 + 64 + 2 * 64 + 2)
#define BRS_POLICY_NVF (64 * 6 + 64 + 64 * 64 + 64 + 1 * 64 + 1)
#define BRS_POLICY_NPARAM (BRS_POLICY_NPI + BRS_POLICY_NVF + 2)

typedef struct brs_policy brs_policy;

int brs_policy_create(int32_t device, brs_policy** out);
int brs_policy_destroy(brs_policy*);
const char* brs_policy_last_error(const brs_policy*);
/* copy BRS_POLICY_NPARAM host floats to the device (synchronous; once per optimiser phase, not per step) */
int brs_policy_set_weights(brs_policy*, const float* params_host);
/* or point at a device-resident parameter vector the learner updates in place (no copy; must stay alive) */
int brs_policy_use_device_weights(brs_policy*, const float* params_dev);

/* one policy step for n envs: action[n][2] (unclipped sample, what the rollout buffer stores), action_clipped[n][2]
 * (clipped to [-1, 1], what brs_step consumes; a NaN action stays NaN, like np.clip, so that brs_step's bad-state guard
 * sees it), logp[n], value[n]; noise[n][2] (the standard normals used) may be NULL.
 * deterministic != 0: action = mean (SB3 predict(deterministic=True)); logp is then that of the mean. */
int brs_policy_act(brs_policy*, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base, uint32_t step,
                   int32_t deterministic, float* action_dev, float* action_clipped_dev, float* logp_dev, float* value_dev,
                   float* noise_dev, void* stream);
/* value head only (e.g. last_values of a rollout) */
int brs_policy_value(brs_policy*, int32_t n, const float* obs_dev, float* value_dev, void* stream);
/* reward[i] += gamma * V(terminal_obs[i]) where truncated[i] && !terminated[i] */
int brs_rollout_bootstrap(brs_policy*, int32_t n, const float* terminal_obs_dev, const uint8_t* terminated_dev,
                          const uint8_t* truncated_dev, float gamma, float* reward_dev, void* stream);
/* GAE(lambda) over a [T][N] rollout: episode_start[t][i] != 0 marks the first step of an episode (SB3's
 * episode_starts); last_value[N] / last_done[N] close the recursion after the final step.  adv and ret are [T][N]. */
int brs_gae(int32_t device, int32_t T, int32_t N, const float* reward_dev, const float* value_dev,
            const uint8_t* episode_start_dev, const float* last_value_dev, const uint8_t* last_done_dev, float gamma,
            float lam, float* adv_dev, float* ret_dev, void* stream);

/* ---- episode statistics.  A monitor watches n envs: brs_monitor_update is called once per env step
 * with the three arrays brs_step wrote (the env's own reward, not a rollout buffer's bootstrapped copy) and keeps, per env,
 * the running return (fp64, summed in step order) and length, and per finished episode the accumulators below, a histogram
 * of episode lengths and -- when targets are set -- a log with one row per counted episode.  Everything lives on the device;
 * no floating-point atomic is used, so two runs on the same inputs return identical bytes. */
typedef struct brs_monitor brs_monitor;

typedef struct brs_episode_stats {
  int64_t episodes;      /* counted episodes: all that ended (no targets), or the first target[i] of env i */
  int64_t ended;         /* episodes that ended, counted or not */
  int64_t terminated;    /* counted episodes that ended with terminated != 0 */
  int64_t time_limit;    /* counted episodes that ended with truncated != 0 and terminated == 0 */
  int64_t sum_len;       /* over counted episodes */
  int64_t sum_len2;
  int64_t steps;         /* brs_monitor_update calls since the last reset */
  double sum_ret;        /* over counted episodes */
  double sum_ret2;
  double min_ret;        /* 0 while no episode is counted */
  double max_ret;
  double running_ret;    /* sum of the returns of the episodes still running */
  int32_t min_len;       /* 0 while no episode is counted */
  int32_t max_len;
  int32_t first_running; /* envs whose first episode has not ended */
  int32_t pending;       /* envs with target[i] > 0 that have not reached it; n without targets */
} brs_episode_stats;

/* max_len: the histogram has bins 1..max_len and bin 0 for longer episodes; log_capacity: rows of the episode log */
int brs_monitor_create(int32_t device, int32_t n, int32_t max_len, int32_t log_capacity, brs_monitor** out);
int brs_monitor_destroy(brs_monitor*);
const char* brs_monitor_last_error(const brs_monitor*);
/* zeroes everything, running episodes included (the caller resets the simulator with it).  targets_host NULL = unlimited;
 * else n entries, each >= 0, their sum <= log_capacity.  Waits for the stream. */
int brs_monitor_reset(brs_monitor*, const int32_t* targets_host, void* stream);
/* one env step of all n envs; only enqueues, no allocation */
int brs_monitor_update(brs_monitor*, const float* reward_dev, const uint8_t* terminated_dev,
                       const uint8_t* truncated_dev, void* stream);
/* reduce kernel + one small device-to-host copy; waits for the stream */
int brs_monitor_stats(brs_monitor*, brs_episode_stats* out_host, void* stream);
/* hist_host has max_len + 1 entries */
int brs_monitor_histogram(brs_monitor*, int64_t* hist_host, void* stream);
/* the sum(targets) rows of the log: episode k of env i is row base[i] + k, base = exclusive prefix sum of the targets;
 * a row that is not filled yet has length 0 */
int brs_monitor_episodes(brs_monitor*, int32_t* env_host, double* ret_host, int32_t* len_host,
                         uint8_t* time_limit_host, void* stream);

/* ---- PPO learner: the minibatch body of SB3's PPO.train() / tools/train_ppo_torch.py::train on the device.
 * brs_learner_grad computes the gradient of the mean loss of one minibatch, brs_learner_apply clips it by norm and takes one
 * torch.optim.Adam step; they are two calls so that a data-parallel caller can all-reduce (and divide) the gradient buffer in
 * between.  Every call only enqueues on `stream`, nothing is allocated after create, all arrays are device pointers owned by
 * the caller.  No floating-point atomic and no communication between workgroups inside a kernel: two runs on the same inputs
 * return identical bytes.  A null handle or a null config is BRS_ERR_ARG (brs_learner_destroy: BRS_ERR_STATE, as everywhere). */
#define BRS_LEARNER_NSTAT 5 /* minibatch means after the gradient: policy loss, value loss, entropy, approx KL, clip fraction */

typedef struct brs_learner brs_learner;

typedef struct brs_ppo_config {
  double lr, beta1, beta2, eps; /* torch.optim.Adam (no amsgrad, no weight decay); fp64 as torch holds them in Python floats */
  float clip_range;
  float vf_coef;
  float ent_coef;
  float max_grad_norm_pi;      /* clip_grad_norm_ of actor + log_std; of everything when joint_norm != 0 */
  float max_grad_norm_vf;      /* ... of the critic (unused when joint_norm != 0) */
  float target_kl;             /* <= 0: no early stop */
  float ret_scale;             /* the value target is ret / ret_scale */
  int32_t normalize_adv;       /* (adv - mean) / (unbiased std + 1e-8) over the minibatch */
  int32_t actor_on;            /* 0: loss = vf_coef * value loss only (critic warm-up); actor and log_std gradients are zero */
  int32_t joint_norm;          /* 1: one global norm (SB3); 0: actor + log_std and critic clipped separately */
} brs_ppo_config;

typedef struct brs_learner_info {
  int64_t steps;       /* Adam steps taken */
  int32_t stopped;     /* sticky: an apply saw approx KL > 1.5 target_kl; cleared by brs_learner_begin_iteration */
  int32_t bad_index;   /* entries of the last idx outside [0, n_rows): they were left out, the gradient is not to be used */
  float stat[BRS_LEARNER_NSTAT]; /* of the gradient buffer the last apply saw */
  float grad_norm_pi;  /* before clipping; the global norm in both when joint_norm != 0 */
  float grad_norm_vf;
} brs_learner_info;

/* max_workgroups <= 0: one per compute unit; > 0 caps the grid of the gradient kernel (each workgroup loops over 256-sample chunks) */
int brs_learner_create(int32_t device, int32_t max_workgroups, brs_learner** out);
int brs_learner_destroy(brs_learner*);
const char* brs_learner_last_error(const brs_learner*);
/* clears the stopped flag (start of a PPO iteration) */
int brs_learner_begin_iteration(brs_learner*, void* stream);
/* params_dev[BRS_POLICY_NPARAM] in the order above; obs[n_rows][6], act[n_rows][2], logp_old, adv, ret [n_rows]: the flat
 * rollout; idx[m] int32 rows of the minibatch (repeats allowed), m >= 2.  Writes grad_dev[BRS_POLICY_NPARAM + BRS_LEARNER_NSTAT]:
 * the gradient of the mean loss, then the BRS_LEARNER_NSTAT means. */
int brs_learner_grad(brs_learner*, const float* params_dev, int32_t n_rows, const float* obs_dev, const float* act_dev,
                     const float* logp_old_dev, const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t m,
                     const brs_ppo_config* cfg, float* grad_dev, void* stream);
/* scale = min(1, max_norm / (norm + 1e-6)), then one Adam step on params / m / v [BRS_POLICY_NPARAM] in place, unless stopped */
int brs_learner_apply(brs_learner*, float* params_dev, const float* grad_dev, float* m_dev, float* v_dev,
                      const brs_ppo_config* cfg, void* stream);
/* one small device-to-host copy; waits for the stream */
int brs_learner_stats(brs_learner*, brs_learner_info* out_host, void* stream);

/* ---- A2C on the same handle: SB3's A2C.train() -- ONE optimiser step on the whole rollout, M = n_steps x n_envs
 * rows in buffer order -- as brs_a2c_grad (the gradient of the mean of -adv log pi(a | s) + vf_coef x value loss - ent_coef x entropy)
 * and brs_a2c_apply (clip_grad_norm_, then SB3's RMSpropTFLike).  The n-step returns and advantages are brs_gae's at lambda = 1.
 * The value loss is the PPO learner's, 0.5 (v - ret / ret_scale)^2 per sample: SB3's vf_coef = 0.5 on mse_loss is vf_coef = 1.0 here;
 * the reported value loss stays 0.5 mean(d^2).  Same rules as above (enqueue only, no allocation, no floating-point atomic, identical
 * bytes from identical inputs, argument errors are BRS_ERR_ARG); brs_learner_stats serves both algorithms, `stopped` is not used. */
typedef struct brs_a2c_config {
  double lr, alpha, eps;       /* RMSpropTFLike: square_avg = alpha square_avg + (1 - alpha) g^2, p -= lr g / sqrt(square_avg + eps) */
  float vf_coef;
  float ent_coef;
  float max_grad_norm_pi;      /* as in brs_ppo_config */
  float max_grad_norm_vf;
  float ret_scale;
  int32_t normalize_adv;       /* (adv - mean) / (unbiased std + 1e-8) over the m rows; needs m >= 2 */
  int32_t actor_on;
  int32_t joint_norm;
} brs_a2c_config;

/* The arrays are brs_learner_grad's, without logp_old.  idx_dev NULL: rows 0..m-1 of the buffer, m <= n_rows.  m >= 1 (m >= 2
 * with normalize_adv).  Writes grad_dev[BRS_POLICY_NPARAM + BRS_LEARNER_NSTAT]: the gradient of the mean loss, then the means of
 * policy loss, value loss and entropy, then two zeros (the KL and clip-fraction slots).  Everything in it is a mean: a
 * data-parallel caller all-reduces and divides it between the two calls. */
int brs_a2c_grad(brs_learner*, const float* params_dev, int32_t n_rows, const float* obs_dev, const float* act_dev,
                 const float* adv_dev, const float* ret_dev, const int32_t* idx_dev, int32_t m, const brs_a2c_config* cfg,
                 float* grad_dev, void* stream);
/* the clip scale of brs_learner_apply, then one RMSpropTFLike step on params / sq [BRS_POLICY_NPARAM] in place; a fresh optimiser's
 * sq is all ONES.  Counts brs_learner_info.steps; there is no early stop */
int brs_a2c_apply(brs_learner*, float* params_dev, const float* grad_dev, float* sq_dev, const brs_a2c_config* cfg, void* stream);

/* ---- DDPG data path: everything SB3's DDPG does between two gradient steps.  The networks are SB3's TD3Policy
 * with the reference's net_arch, widths fixed at compile time; each is a flat fp32 device vector, torch.nn.Linear layout:
 *   actor : W1[300][6] b1[300] W2[200][300] b2[200] W3[2][200] b3[2], ReLU ReLU tanh   (actor.mu.0/.2/.4.{weight,bias})
 *   critic: W1[200][8] b1[200] W2[150][200] b2[150] W3[1][150] b3[1], ReLU ReLU linear (critic.qf0.0/.2/.4.{weight,bias}),
 *           input = concat(obs[6], action[2])
 * The parameter vectors are arguments of every call (read in place: the caller's optimiser and Polyak update write them).  Every
 * call only enqueues on `stream`, nothing is allocated after create, no floating-point atomic: two runs on the same inputs
 * return identical bytes.  The forwards run in fp32 on the matrix cores; hidden activations stay on the chip. */
#define BRS_DDPG_NACTOR (300 * 6 + 300 + 200 * 300 + 200 + 2 * 200 + 2)  /* 62,702 */
#define BRS_DDPG_NCRITIC (200 * 8 + 200 + 150 * 200 + 150 + 1 * 150 + 1) /* 32,101 */
#define BRS_DDPG_TAG_ACT 0x44445047u    /* "DDPG": second Philox counter word of brs_ddpg_act */
#define BRS_DDPG_TAG_SAMPLE 0x5245504cu /* "REPL": ... of brs_replay_sample */

typedef struct brs_ddpg brs_ddpg;

int brs_ddpg_create(int32_t device, brs_ddpg** out);
int brs_ddpg_destroy(brs_ddpg*);
const char* brs_ddpg_last_error(const brs_ddpg*);
/* SB3's _sample_action for n envs.  mean = actor(obs), or with random != 0 (the learning_starts phase) a uniform draw per
 * component; action = clip(mean + sigma z, -1, 1) in both modes (SB3 adds the action noise during warm-up too); sigma == 0 is
 * predict(deterministic=True).  One action: what the buffer stores is what the env consumes.  mean_dev and noise_dev [n][2] may
 * be NULL.  Randomness: Philox4x32-10(counter = (step, BRS_DDPG_TAG_ACT, gid_lo, gid_hi), key = seed), gid = env_index_base + i;
 * words 0 and 1 -> z[0], z[1] by the Box-Muller of brs_policy_act (u = ((w >> 8) + 0.5) / 2^24, r = sqrt(-2 ln u1),
 * z = r cos / sin(2 pi u2)); words 2 and 3 -> the uniform components, ((w >> 8) - 2^23) / 2^23 in [-1, 1 - 2^-23]. */
int brs_ddpg_act(brs_ddpg*, const float* actor_dev, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base,
                 uint32_t step, float sigma, int32_t random, float* action_dev, float* mean_dev, float* noise_dev, void* stream);
/* q[n] = critic(concat(obs[n][6], act[n][2])) */
int brs_ddpg_q(brs_ddpg*, const float* critic_dev, int32_t n, const float* obs_dev, const float* act_dev, float* q_dev, void* stream);
/* y[m] = reward + (1 - done) gamma Q'(next_obs, pi'(next_obs)) from the two TARGET networks, one launch; a row with done != 0
 * gets y == reward exactly */
int brs_ddpg_td_target(brs_ddpg*, const float* actor_target_dev, const float* critic_target_dev, int32_t m, const float* next_obs_dev,
                       const float* reward_dev, const uint8_t* done_dev, float gamma, float* y_dev, void* stream);

/* Replay buffer: the caller owns the storage, time is the major axis as in SB3: obs[cap][n][6], next_obs[cap][n][6],
 * action[cap][n][2], reward[cap][n], done[cap][n].  The same struct names the five contiguous [m]-leading outputs of a sample.
 * No handle: errors go to a per-thread slot (brs_replay_last_error).  cap * n <= 2^31 - 1; offsets are 64-bit. */
typedef struct brs_replay_storage {
  float* obs;
  float* next_obs;
  float* action;
  float* reward;
  uint8_t* done;
} brs_replay_storage;

/* writes row pos (0 <= pos < cap; the caller advances it modulo cap) from one env step: last_obs (what the action was computed
 * from), the action, and brs_step's five outputs.  next_obs[i] = terminal_obs[i] where terminated[i] | truncated[i], else
 * obs[i]; done[i] = terminated[i] != 0 (SB3: dones * (1 - timeouts)): a time-limit end bootstraps, a fall does not. */
int brs_replay_add(int32_t device, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t pos, const float* last_obs_dev,
                   const float* action_dev, const float* obs_dev, const float* reward_dev, const uint8_t* terminated_dev,
                   const uint8_t* truncated_dev, const float* terminal_obs_dev, void* stream);
/* m uniform samples from the first `size` rows (1 <= size <= cap: pos until the first wrap, then cap), index and gather in one
 * kernel.  Sample j takes Philox4x32-10(counter = (draw, BRS_DDPG_TAG_SAMPLE, j, 0), key = seed): row = (w0 * size) >> 32,
 * env = (w1 * n) >> 32, two independent draws as SB3 makes them; the probability of a cell deviates from 1 / (size n) by at most
 * n / 2^32 relative (size / 2^32 for the row).  idx_dev [m][2] int32 (row, env) may be NULL. */
int brs_replay_sample(int32_t device, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t size, int32_t m,
                      uint64_t seed, uint32_t draw, const brs_replay_storage* out, int32_t* idx_dev, void* stream);
const char* brs_replay_last_error(void);

/* ---- TD3's target: y[m] = reward + (1 - done) gamma min(Q1'(s', a'), Q2'(s', a')) with
 * a' = clamp(pi'(s') + clamp(policy_noise z, -noise_clip, noise_clip), -1, 1), all from the three TARGET networks, one launch;
 * critics_target_dev holds the two critics back to back.  A row with done != 0 gets y == reward exactly.  Row j takes
 * Philox4x32-10(counter = (draw, BRS_TD3_TAG_NOISE, j, 0), key = seed); words 0 and 1 -> z[0], z[1] by brs_ddpg_act's Box-Muller.
 * next_action_dev [m][2] (a') and noise_dev [m][2] (z, before the scale and the clip) may be NULL.  policy_noise and noise_clip
 * are finite and >= 0; policy_noise == 0 with two equal critics is brs_ddpg_td_target byte for byte. */
#define BRS_TD3_TAG_NOISE 0x5444334eu /* "TD3N": second Philox counter word of brs_td3_td_target */
int brs_td3_td_target(brs_ddpg*, const float* actor_target_dev, const float* critics_target_dev, int32_t m, const float* next_obs_dev,
                      const float* reward_dev, const uint8_t* done_dev, float gamma, float policy_noise, float noise_clip, uint64_t seed,
                      uint32_t draw, float* y_dev, float* next_action_dev, float* noise_dev, void* stream);

/* ---- DDPG learner: the gradient step between two TD targets.  SB3's order is critic_grad, apply (critic),
 * actor_grad WITH THE UPDATED CRITIC, apply (actor); the Polyak update of a network is fused into its own apply (the critic
 * target is read only by the next brs_ddpg_td_target).  grad and apply are separate calls so that a data-parallel caller can
 * all-reduce-and-divide the buffer in between: all three calls write MEANS over the m rows.  The handle owns the scratch that
 * max_batch rows need ([unit][sample] images of the activations and their gradients); calls on one handle must be ordered on
 * one stream.  Every call only enqueues, nothing is allocated after create, no floating-point atomic, no communication between
 * workgroups: two runs on the same inputs return identical bytes.  Arguments are checked before a device is looked for. */
#define BRS_DDPG_NSTAT 2
typedef struct brs_ddpg_learner brs_ddpg_learner;
typedef struct brs_adam_config { double lr, beta1, beta2, eps; } brs_adam_config; /* fp64, as torch holds them */

int brs_ddpg_learner_create(int32_t device, int32_t max_batch, brs_ddpg_learner** out);
int brs_ddpg_learner_destroy(brs_ddpg_learner*);
const char* brs_ddpg_learner_last_error(const brs_ddpg_learner*);
/* the handle's one device allocation (activation images, then the partial rows) and its size: memory accounting, and the tests
 * fill it with NaN before a call to show that a call reads nothing it has not written itself.  Enqueues nothing. */
int brs_ddpg_learner_scratch(brs_ddpg_learner*, void** scratch_dev, int64_t* bytes);
/* grad_dev[BRS_DDPG_NCRITIC + 2]: gradient of Lc = mean_i (Q(s_i, a_i) - y_i)^2 in the critic's flat order, then Lc and
 * mean_i Q(s_i, a_i); 1 <= m <= max_batch */
int brs_ddpg_learner_critic_grad(brs_ddpg_learner*, const float* critic_dev, int32_t m, const float* obs_dev, const float* act_dev,
                                 const float* y_dev, float* grad_dev, void* stream);
/* grad_dev[BRS_DDPG_NACTOR + 2]: gradient of La = -mean_i Q(s_i, pi(s_i)) in the actor's flat order, then La and the mean of
 * pi(s)^2 over rows and both components (how saturated the tanh is).  The critic's weights get no gradient. */
int brs_ddpg_learner_actor_grad(brs_ddpg_learner*, const float* actor_dev, const float* critic_dev, int32_t m, const float* obs_dev,
                                float* grad_dev, void* stream);
/* torch.optim.Adam (no amsgrad, no weight decay) on params / m / v in place from grad_dev[0 .. n_param), step counted from 1 by
 * the CALLER (bias corrections formed in fp64 on the host); then, if target_dev is not NULL,
 * target += tau * (params_new - target).  Element-wise: any n_param >= 1.  step >= 1, 0 <= tau <= 1, lr and eps >= 0, betas in
 * [0, 1). */
int brs_ddpg_learner_apply(brs_ddpg_learner*, int32_t n_param, float* params_dev, const float* grad_dev, float* m_dev, float* v_dev,
                           float* target_dev, const brs_adam_config* cfg, int64_t step, float tau, void* stream);

/* ---- TD3's twin critics.  A handle from brs_ddpg_learner_create_twin serves every call above unchanged and has
 * the scratch and the partial rows for two critics at once; brs_ddpg_learner_create's handles stay as they are.
 * grad_dev[2 * BRS_DDPG_NCRITIC + BRS_TD3_NSTAT]: critic 0's gradient of mse(Q1(s, a), y) in its flat order, then critic 1's of
 * mse(Q2(s, a), y) -- the gradient of the summed loss w.r.t. one critic is that of its own term -- then Lc and mean Q of critic 0,
 * Lc and mean Q of critic 1.  Block k and its two statistics are byte for byte what brs_ddpg_learner_critic_grad returns for
 * critic k alone.  One brs_ddpg_learner_apply with n_param = 2 * BRS_DDPG_NCRITIC is the Adam (and Polyak) step of both. */
#define BRS_TD3_NSTAT 4
int brs_ddpg_learner_create_twin(int32_t device, int32_t max_batch, brs_ddpg_learner** out);
int brs_ddpg_learner_twin_critic_grad(brs_ddpg_learner*, const float* critics_dev, int32_t m, const float* obs_dev, const float* act_dev,
                                      const float* y_dev, float* grad_dev, void* stream);

/* ---- SAC on the same widths: SB3's SACPolicy / SAC.train with pi=[300, 200], qf=[200, 150].
 *   SAC actor: W1[300][6] b1[300] W2[200][300] b2[200] W3[4][200] b3[4], ReLU ReLU linear; output rows 0-1 are actor.mu, rows 2-3
 *              actor.log_std (two Linear(200, 2) stacked).  The actor VECTOR has BRS_SAC_NACTOR + 1 elements: the last one is
 *              log_ent_coef, and every SAC kernel that needs the temperature reads alpha = exp(actor[BRS_SAC_NACTOR]) from device
 *              memory.  brs_sac_act does not read that element.
 *   critics  : two DDPG critics back to back [2 BRS_DDPG_NCRITIC], as TD3's; only the critics have targets.
 * With sigma = exp(clamp(log_std, -20, 2)), u = mu + sigma z and a = tanh(u):
 *   logp = sum_k (-z_k^2 / 2 - log_std_k - log(2 pi) / 2) - sum_k log(1 - a_k^2 + 1e-6)     (log_std clamped; 1 - a^2 from the
 *   exponential of the tanh, so that it does not cancel where the tanh saturates) */
#define BRS_SAC_NACTOR (300 * 6 + 300 + 200 * 300 + 200 + 4 * 200 + 4) /* 63,104 */
#define BRS_SAC_NSTAT 4
#define BRS_SAC_TAG_ACT 0x53414341u    /* "SACA": second Philox counter word of brs_sac_act */
#define BRS_SAC_TAG_TARGET 0x53414354u /* "SACT": ... of brs_sac_td_target */
#define BRS_SAC_TAG_PI 0x53414350u     /* "SACP": ... of brs_sac_actor_grad */

/* SB3's SAC actor for n envs, brs_ddpg_act's contract: action = tanh(mu + sigma z) with z[0], z[1] from words 0 and 1 of
 * Philox4x32-10(counter = (step, BRS_SAC_TAG_ACT, gid_lo, gid_hi), key = seed), gid = env_index_base + i, by brs_ddpg_act's
 * Box-Muller; deterministic != 0: action = tanh(mu); random != 0 (the learning_starts phase; actor_dev and obs_dev may be NULL):
 * the uniform components of words 2 and 3, and then mu = action, log_std = 0.  mu_dev, log_std_dev (clamped) and z_dev [n][2] may
 * be NULL. */
int brs_sac_act(brs_ddpg*, const float* actor_dev, int32_t n, const float* obs_dev, uint64_t seed, int64_t env_index_base, uint32_t step,
                int32_t deterministic, int32_t random, float* action_dev, float* mu_dev, float* log_std_dev, float* z_dev, void* stream);
/* y[m] = reward + (1 - done) gamma (min(Q1', Q2')(s', a') - alpha logp') in one launch: the CURRENT actor on next_obs (SAC has
 * no target actor), row j's z from Philox4x32-10(counter = (draw, BRS_SAC_TAG_TARGET, j, 0), key = seed), the two TARGET critics.
 * A row with done != 0 gets y == reward exactly.  next_action_dev [m][2] (a'), logp_dev [m] (logp') and z_dev [m][2] may be NULL. */
int brs_sac_td_target(brs_ddpg*, const float* actor_dev, const float* critics_target_dev, int32_t m, const float* next_obs_dev,
                      const float* reward_dev, const uint8_t* done_dev, float gamma, uint64_t seed, uint32_t draw, float* y_dev,
                      float* next_action_dev, float* logp_dev, float* z_dev, void* stream);
/* A handle of the brs_ddpg_learner family with room for the SAC calls below: every brs_ddpg_learner_* call works on it, and the
 * handles of brs_ddpg_learner_create / _create_twin stay as they are.  The SAC calls refuse any other handle. */
int brs_ddpg_learner_create_sac(int32_t device, int32_t max_batch, brs_ddpg_learner** out);
/* SB3's critic_loss = 0.5 (mse(Q1, y) + mse(Q2, y)): brs_ddpg_learner_twin_critic_grad's buffer with every parameter block and the
 * two loss statistics multiplied by 0.5 (exactly: a power of two at the loss head); the two mean Q stay. */
int brs_sac_twin_critic_grad(brs_ddpg_learner*, const float* critics_dev, int32_t m, const float* obs_dev, const float* act_dev,
                             const float* y_dev, float* grad_dev, void* stream);
/* grad_dev[BRS_SAC_NACTOR + 1 + BRS_SAC_NSTAT]: the gradient of La = mean_i (alpha logp_i - min(Q1, Q2)(s_i, a_i)) in the SAC
 * actor's flat order, a_i sampled with row i's z from Philox4x32-10(counter = (draw, BRS_SAC_TAG_PI, i, 0), key = seed), through
 * both critics (which get no gradient; per row the smaller Q takes it, critic 0 on a tie); element BRS_SAC_NACTOR:
 * learn_alpha != 0 ? -(mean logp + target_entropy) : 0, SB3's ent_coef_loss differentiated by log_ent_coef, so that one
 * brs_ddpg_learner_apply with n_param = BRS_SAC_NACTOR + 1 steps the actor and the temperature (a zero gradient leaves an element
 * of Adam at zero moments unchanged); then La, mean logp, mean min Q and alpha. */
int brs_sac_actor_grad(brs_ddpg_learner*, const float* actor_dev, const float* critics_dev, int32_t m, const float* obs_dev, uint64_t seed,
                       uint32_t draw, int32_t learn_alpha, float target_entropy, float* grad_dev, void* stream);

/* ---- network architectures.  The widths of a brs_ddpg / brs_ddpg_learner handle are those of its architecture,
 * fixed at create; every call on the handle takes and returns vectors of that architecture's lengths, its contract otherwise
 * unchanged.
 *   BRS_ARCH_REFERENCE   pi=[300, 200], qf=[200, 150]: the reference's DDPG net_arch, everything above; what brs_ddpg_create and
 *                        brs_ddpg_learner_create / _create_twin / _create_sac make.
 *   BRS_ARCH_SAC_DEFAULT net_arch=[256, 256] for the actor and both critics: SB3's SAC("MlpPolicy", env).
 *     SAC actor: W1[256][6] b1[256] W2[256][256] b2[256] W3[4][256] b3[4], then log_ent_coef   [BRS_SAC256_NACTOR + 1]
 *     critic   : W1[256][8] b1[256] W2[256][256] b2[256] W3[1][256] b3[1]                      [BRS_SAC256_NCRITIC], two back to back
 * An arch-1 handle serves the SAC calls -- brs_sac_act, brs_sac_td_target, brs_ddpg_q, brs_sac_twin_critic_grad, brs_sac_actor_grad,
 * brs_ddpg_learner_apply, brs_ddpg_learner_scratch -- with BRS_SAC256_* in the place of BRS_SAC_NACTOR and BRS_DDPG_NCRITIC.  SB3 has
 * no DDPG or TD3 at these widths: brs_ddpg_act, brs_ddpg_td_target, brs_td3_td_target, brs_ddpg_learner_critic_grad,
 * _twin_critic_grad and _actor_grad return BRS_ERR_ARG on it and enqueue nothing.  An unknown arch is BRS_ERR_ARG. */
#define BRS_ARCH_REFERENCE 0
#define BRS_ARCH_SAC_DEFAULT 1
#define BRS_SAC256_NACTOR (256 * 6 + 256 + 256 * 256 + 256 + 4 * 256 + 4)  /* 68,612 */
#define BRS_SAC256_NCRITIC (256 * 8 + 256 + 256 * 256 + 256 + 1 * 256 + 1) /* 68,353 */
int brs_ddpg_create_arch(int32_t device, int32_t arch, brs_ddpg** out);
int brs_ddpg_learner_create_sac_arch(int32_t device, int32_t max_batch, int32_t arch, brs_ddpg_learner** out);

/* ---- VecNormalize: SB3's VecNormalize / RunningMeanStd for the n envs of a simulator, on the device.  Per
 * column -- the six observation columns and the discounted return -- a running mean, variance and count in fp64 (0, 1, 1e-4 at
 * create), and per env the discounted return (fp64, 0 at create).  A batch enters as its (count, mean, M2) triple, reduced by a
 * tree of Chan merges whose shape depends on n alone (no atomics): the statistics are the same bytes on every run.
 *   batch update   delta = bm - mean; tot = count + n; mean += delta n / tot;
 *                  var = (var count + bv n + delta^2 count n / tot) / tot; count = tot
 *   normalise      obs_out = clip((obs - mean) / sqrt(var + epsilon), +-clip_obs); reward_out = clip(reward / sqrt(ret_var +
 *                  epsilon), +-clip_reward); evaluated in fp64, rounded once to fp32; a NaN stays a NaN; norm_obs == 0 /
 *                  norm_reward == 0 copy the input through */
typedef struct brs_vecnorm brs_vecnorm;

typedef struct brs_vecnorm_config {
  double gamma;        /* discount of the return the reward statistics are taken of (0.99) */
  double epsilon;      /* 1e-8 */
  double clip_obs;     /* >= 0 (10) */
  double clip_reward;  /* >= 0 (10) */
  int32_t norm_obs;
  int32_t norm_reward;
} brs_vecnorm_config;

typedef struct brs_vecnorm_stats {
  double obs_mean[6], obs_var[6], obs_count[6];
  double ret_mean, ret_var, ret_count;
} brs_vecnorm_stats;

int brs_vecnorm_create(int32_t device, int32_t n, const brs_vecnorm_config* config, brs_vecnorm** out);
int brs_vecnorm_destroy(brs_vecnorm*);
const char* brs_vecnorm_last_error(const brs_vecnorm*);
/* returns = 0; with training && norm_obs the observation statistics take obs_dev [n][6]; obs_out_dev [n][6] receives the
 * normalised observations.  Only enqueues. */
int brs_vecnorm_reset(brs_vecnorm*, const float* obs_dev, int32_t training, float* obs_out_dev, void* stream);
/* one env step, in this order: with training && norm_obs the observation statistics take obs_dev; with training
 * returns = returns gamma + reward and the return statistics take returns; the three outputs are written with the updated
 * statistics (terminal_obs_out_dev: every row of terminal_obs_dev [n][6]); returns[i] = 0 where terminated[i] | truncated[i],
 * training or not.  Only enqueues, no allocation.  An output may not alias an input. */
int brs_vecnorm_step(brs_vecnorm*, const float* obs_dev, const float* reward_dev, const uint8_t* terminated_dev,
                     const uint8_t* truncated_dev, const float* terminal_obs_dev, int32_t training, float* obs_out_dev,
                     float* reward_out_dev, float* terminal_obs_out_dev, void* stream);
/* any m >= 1, no state touched: in_dev / out_dev [m][6] and [m].  Only enqueue. */
int brs_vecnorm_normalize_obs(brs_vecnorm*, int32_t m, const float* in_dev, float* out_dev, void* stream);
int brs_vecnorm_normalize_reward(brs_vecnorm*, int32_t m, const float* in_dev, float* out_dev, void* stream);
/* VecNormalize.save / .load: the 21 doubles, and returns [n].  get_* wait for the stream; set_stats only enqueues a copy of
 * *in_host, which is read before the call returns */
int brs_vecnorm_get_stats(brs_vecnorm*, brs_vecnorm_stats* out_host, void* stream);
int brs_vecnorm_set_stats(brs_vecnorm*, const brs_vecnorm_stats* in_host, void* stream);
int brs_vecnorm_get_returns(brs_vecnorm*, double* returns_host, void* stream);

/* ---- VecNormalize for the off-policy family.  SB3's rule: the actor acts on the normalised observation, the
 * replay buffer stores the RAW observation, next observation and reward, and ReplayBuffer.sample(batch_size, env=vec_normalize)
 * normalises the minibatch with the statistics of the moment of sampling.
 * brs_replay_sample_vecnorm: brs_replay_sample's cells (the same Philox block, the same row/env map, the same idx), with obs and
 * next_obs through normalize_obs and reward through normalize_reward of the handle's CURRENT statistics; action and done copied.
 * One launch: every output byte is what brs_replay_sample followed by brs_vecnorm_normalize_obs (twice) and
 * brs_vecnorm_normalize_reward writes.  Reads the statistics, writes neither them nor the returns nor the storage.  norm_obs == 0 /
 * norm_reward == 0 copy that half through.  `n` is the buffer's env count and need not be the handle's.  The argument conditions
 * are brs_replay_sample's (idx_dev may be null).  Only enqueues.  Errors go to the handle's slot (brs_vecnorm_last_error); a null
 * handle returns BRS_ERR_STATE. */
int brs_replay_sample_vecnorm(brs_vecnorm*, const brs_replay_storage* storage, int32_t n, int32_t cap, int32_t size, int32_t m,
                              uint64_t seed, uint32_t draw, const brs_replay_storage* out, int32_t* idx_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
