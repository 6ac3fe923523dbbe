/*
 * brs_qpolicy.h -- C ABI of the int8 actor: the deployment check at the end of the reference's pipeline.  The reference
 * quantises a trained policy to int8 (src/quantize_tflite.py) and then drives the int8 network in closed loop in the
 * simulator through the TFLite interpreter, one env at a time, before the file is flashed to the Arduino
 * (src/sb_rl.py:285-364, `test-tflite-quant`).  These entry points evaluate such a network for n envs on the GPU, next to
 * brs_step, with integer arithmetic only: the result is the same on every platform, bit for bit.
 *
 * The network is the actor tower of SB3's MlpPolicy, 6 -> 64 -> tanh -> 64 -> tanh -> 2.  Per layer k: int8 weights
 * W[out][in], int32 bias b[out], a real multiplier per output channel M[c] = bias_scale[c] / out_scale, an output zero
 * point oz; hidden layers have a 256-entry int8 tanh table.
 *
 *   1. input        q0 = clamp(rint((double)obs / input_scale) + input_zero, -128, 127)   (IEEE fp64 division, half to
 *                   even; NaN -> input_zero, +-Inf saturates; clamped before the conversion to an integer)
 *   2. accumulate   acc[c] = b[c] + sum_i W[c][i] (q_in[i] - z_in) in int32.  The library folds -z_in sum_i W[c][i] into
 *                   the bias once, at brs_qpolicy_set_model (exact), and the kernel multiplies int8 by int8.
 *   3. requantise   M = m 2^-t with m in [2^30, 2^31) (brs_qpolicy_quantize_multiplier), ONE rounding:
 *                   q = clamp((((int64)acc m + (1 << (t - 1))) >> t) + oz, -128, 127), arithmetic shift
 *   4. tanh         q <- table[q + 128]; the table is made by the caller, the device evaluates no transcendental
 *   5. output       action = (float)((double)(q2 - oz2) out_scale2), not clipped (brs_step does not clip either, and the
 *                   reference passes the raw output to env.step); the int8 code q2 is available too
 *
 * Same library (libbrs_hip.so), same status codes as brs.h.  Parity with the TFLite interpreter itself is not claimed:
 * its double-rounding multiplier and its own table can differ from the above by one int8 step on a tie.
 */
#ifndef BRS_QPOLICY_H
#define BRS_QPOLICY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRS_QPOLICY_OBS 6
#define BRS_QPOLICY_HID 64
#define BRS_QPOLICY_ACT 2

typedef struct brs_qlayer {
  int32_t n_in, n_out;       /* 6/64, 64/64, 64/2 */
  const int8_t* weight;      /* [n_out][n_in] */
  const int32_t* bias;       /* [n_out], as exported (the zero point of the input is NOT folded in) */
  const double* bias_scale;  /* [n_out]: scale of the layer's input x scale of the channel's weights */
  double out_scale;          /* scale of the layer's int8 output (before the tanh table) */
  int32_t out_zero;          /* its zero point, in [-128, 127] */
  int32_t tanh_zero;         /* zero point of the table's OUTPUT = of the next layer's input; ignored without a table */
  const int8_t* tanh_table;  /* [256], indexed by q + 128; NULL on the output layer only */
} brs_qlayer;

typedef struct brs_qmodel {
  double input_scale;  /* of the observation */
  int32_t input_zero;
  int32_t reserved;    /* 0 */
  brs_qlayer layer[3]; /* the output scale and zero point are layer[2].out_scale / .out_zero */
} brs_qmodel;

typedef struct brs_qpolicy brs_qpolicy;

/* replaces the tf.lite.Interpreter(...) / allocate_tensors() of sb_rl.py:306-307; needs a HIP device */
int brs_qpolicy_create(int32_t device, brs_qpolicy** out);
int brs_qpolicy_destroy(brs_qpolicy*);
const char* brs_qpolicy_last_error(const brs_qpolicy*);

/* step 3's decomposition, the one definition of it (host only, no device needed): (f, e) = frexp(M),
 * m = round(f 2^31), m == 2^31 -> m = 2^30 and e + 1, t = 31 - e.  BRS_ERR_ARG for M <= 0, a non-finite M, or t outside
 * [1, 62]. */
int brs_qpolicy_quantize_multiplier(double M, int32_t* m, int32_t* t);

/* load a model (all pointers in it are HOST pointers; nothing is kept).  Checked, each failure is BRS_ERR_ARG: the sizes
 * are exactly 6/64/64/2, hidden layers have a table and the output layer has none, every zero point is in [-128, 127],
 * every multiplier is valid, and no int8 input can take an accumulator (with or without the folded zero point) out of
 * int32.  Weights of -128 are allowed.  The model is checked BEFORE the handle is looked at, so a model can be checked
 * without a device: with a NULL handle a bad model gives BRS_ERR_ARG and a good one BRS_ERR_STATE.  Synchronous, like
 * brs_policy_set_weights: it drains the device, then copies.  Replaces the interpreter's reading of the .tflite file
 * (sb_rl.py:306-324). */
int brs_qpolicy_set_model(brs_qpolicy*, const brs_qmodel*);

/* one step of the int8 network for n envs, sb_rl.py:331-357 for all of them at once: obs[n][6] floats as brs_step
 * wrote them -> action[n][2] floats for brs_step, and the int8 codes action_q[n][2] (may be NULL).  Device pointers;
 * only enqueues on `stream`: no synchronisation, no allocation, capturable into a graph like brs_render. */
int brs_qpolicy_act(brs_qpolicy*, int32_t n, const float* obs_dev, float* action_dev, int8_t* action_q_dev, void* stream);

/*
 * The int8 form of the OFF-POLICY actor, the network DDPG, TD3 and SAC train (include/brs_policy.h: brs_ddpg_act, and
 * the deterministic action tanh(mu) of brs_sac_act):
 *
 *     obs[6] -> 300 -> ReLU -> 200 -> ReLU -> 2 -> tanh
 *
 * Hidden layers carry NO table (tanh_table == NULL, tanh_zero ignored); the output layer carries one.  Steps, each
 * defined so that every platform gives the same bits:
 *
 *   1. input        as step 1 above
 *   2. accumulate   acc[c] = b[c] + sum_i W[c][i] (q_in[i] - z_in) in int32.  z_in of layer 0 is input_zero, of layers 1
 *                   and 2 the previous layer's out_zero: there is no table in between, so the previous layer's output code
 *                   IS the next layer's input code.  The fold into the bias happens once, at set_model, as above.
 *   3. requantise   as step 3 above: one rounding, clamp to [-128, 127]
 *   4. ReLU         hidden layers only: q <- max(q, out_zero), out_zero being the code of real 0
 *   5. tanh         output layer only: q <- table[q + 128], made by the caller; no transcendental on the device
 *   6. output       action = (float)((double)(q - action_zero) action_scale), not clipped; the code q is available too
 *
 * A SECOND NETWORK, the same six steps at other hidden widths: SB3's default net_arch = [256, 256], what its SAC trains,
 *
 *     obs[6] -> 256 -> ReLU -> 256 -> ReLU -> 2 -> tanh
 *
 * (the deterministic action tanh(mu) of a BRS_ARCH_SAC_DEFAULT actor of include/brs_policy.h).  A handle serves ONE of the two
 * networks, fixed when it is created (brs_qpolicy_actor_create_arch); the model struct is the same, its sizes are the network's.
 * Step 2's int32 bound at these widths: K = 256, |sum| <= 256 x 128 x 255 < 2^23, next to the bias.
 *
 * The entry points are named brs_qpolicy_actor_... because every function this header declares belongs to the
 * brs_qpolicy_ family of the library's symbol table.
 */
#define BRS_QACTOR_OBS 6
#define BRS_QACTOR_H0 300
#define BRS_QACTOR_H1 200
#define BRS_QACTOR_ACT 2
#define BRS_QACTOR256_H0 256
#define BRS_QACTOR256_H1 256
/* the architecture of a handle: the values of BRS_ARCH_REFERENCE and BRS_ARCH_SAC_DEFAULT of include/brs_policy.h, which this
 * header does not include (the library asserts that they are equal) */
#define BRS_QACTOR_ARCH_REFERENCE 0
#define BRS_QACTOR_ARCH_SAC_DEFAULT 1

typedef struct brs_qactor_model {
  double input_scale;  /* of the observation */
  int32_t input_zero;
  int32_t action_zero; /* zero point of the output table's result */
  double action_scale; /* its scale */
  brs_qlayer layer[3]; /* 6/300, 300/200, 200/2 (or 6/256, 256/256, 256/2); only layer[2] has a table */
} brs_qactor_model;

typedef struct brs_qactor brs_qactor;

/* needs a HIP device; a handle for the 6-300-200-2 network (BRS_QACTOR_ARCH_REFERENCE) */
int brs_qpolicy_actor_create(int32_t device, brs_qactor** out);
/* the same for the network of `arch`: BRS_QACTOR_ARCH_REFERENCE (6-300-200-2) or BRS_QACTOR_ARCH_SAC_DEFAULT (6-256-256-2).  The
 * handle remembers it.  An unknown arch or a NULL `out` is BRS_ERR_ARG. */
int brs_qpolicy_actor_create_arch(int32_t device, int32_t arch, brs_qactor** out);
int brs_qpolicy_actor_destroy(brs_qactor*);
const char* brs_qpolicy_actor_last_error(const brs_qactor*);

/* load a model (HOST pointers; nothing is kept).  Checked, each failure is BRS_ERR_ARG with a message that names layer
 * and channel: the sizes are exactly 6/300/200/2, the output layer has a table and the hidden layers have none, every
 * zero point is in [-128, 127], every scale is positive and finite, every multiplier is valid, and no int8 input can
 * take an accumulator (with or without the folded zero point) out of int32.  The model is checked BEFORE the handle is
 * looked at: with a NULL handle a bad model gives BRS_ERR_ARG and a good one BRS_ERR_STATE.  Synchronous: it drains the
 * device, then copies.  The sizes are those of the HANDLE's network (with a NULL handle: 6/300/200/2); a model of the other
 * network is BRS_ERR_ARG, and the message names the network the handle serves. */
int brs_qpolicy_actor_set_model(brs_qactor*, const brs_qactor_model*);

/* the checks of brs_qpolicy_actor_set_model for the network of `arch`, and nothing else: host only, no device and no handle.
 * BRS_OK for a model that set_model would load on a handle of that arch; otherwise BRS_ERR_ARG and set_model's message in
 * brs_qpolicy_actor_last_error(NULL).  An unknown arch is BRS_ERR_ARG. */
int brs_qpolicy_actor_check_model(int32_t arch, const brs_qactor_model*);

/* one step of the int8 actor for n envs: obs[n][6] floats -> action[n][2] floats, and the int8 codes action_q[n][2]
 * (may be NULL).  Device pointers; only enqueues on `stream`: no synchronisation, no allocation, capturable into a
 * graph.  Rows beyond n - 1 are never written.  The kernel is the one of the handle's network. */
int brs_qpolicy_actor_act(brs_qactor*, int32_t n, const float* obs_dev, float* action_dev, int8_t* action_q_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
