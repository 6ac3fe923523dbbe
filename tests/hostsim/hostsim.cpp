// hostsim.cpp -- HOST compilation of the kernel source (balance_robot_mujoco_rl_amd/csrc/brs_core.hpp) for tests.
// TEST INFRASTRUCTURE ONLY: lets the CPU test-suite check the fp32 algorithm the HIP kernel runs (and a
// double instantiation of the same closed forms) against oracle/ without a GPU.  Never loaded by the
// product; the product path is libbrs_hip.so and fails loudly without a GPU.
#include <omp.h>

#include <cstring>
#include <memory>
#include <vector>

#include "brs_state.hpp"

using namespace brs;

struct IHost {
  virtual ~IHost() {}
  virtual int nq() const = 0;
  virtual int nv() const = 0;
  virtual void set_state(const double*, const double*, const double*, const double*) = 0;
  virtual void get_state(double*, double*, double*, double*) const = 0;
  virtual void get_aux(double*) const = 0;
  virtual void set_aux(const double*) = 0;
  virtual void get_xpose(double*, double*) const = 0;
  virtual void set_xpose(const double*, const double*) = 0;
  virtual void physics(const double* ctrl, int nsub) = 0;
  virtual void reset(const uint8_t* mask, float* obs) = 0;
  virtual void step(const float* act, float* obs, float* rew, uint8_t* term, uint8_t* trunc, float* tobs) = 0;
  virtual void step_stub(int env, const float* act, const double* qpos, const double* qvel, const double* xquat, const double* xpos,
                         float* obs, float* rew, uint8_t* term, uint8_t* trunc, double* ctrl) = 0;
  virtual void script(int env, const double* u, int n) = 0;
  virtual int script_remaining(int env) const = 0;
  virtual void cost_class(int* key, double* cmp) const = 0;
};

template <typename R, bool BLK> struct HostSim : IHost {
  using L = Layout<BLK>;
  using ES = EnvState<R, BLK>;
  Params<R> P;
  size_t N;
  std::vector<double> d;
  std::vector<R> f;
  std::vector<int> ii;
  std::vector<std::vector<double>> scripts;
  std::vector<int> spos;
  HostSim(int variant, int n, uint64_t seed, int64_t gid_base, int auto_reset, int noise, int max_steps, int nsub, double h)
      : N(n), d((size_t)L::ND * n), f((size_t)L::NF * n), ii((size_t)L::NI * n), scripts(n), spos(n, 0) {
    P = make_params<R>(variant, auto_reset, noise, max_steps, nsub, h, seed, gid_base);
    hostconv::init_state<BLK>(d.data(), f.data(), ii.data(), N, seed, gid_base);
  }
  int nq() const override { return L::NQ; }
  int nv() const override { return L::NV; }
  void set_state(const double* qp, const double* qv, const double* wm, const double* tm) override {
    hostconv::set_state<BLK>(d.data(), f.data(), N, qp, qv, wm, tm);
    hostconv::mark_bad_start<BLK>(d.data(), f.data(), ii.data(), N);
  }
  void get_state(double* qp, double* qv, double* wm, double* tm) const override {
    hostconv::get_state<BLK>(d.data(), f.data(), N, qp, qv, wm, tm);
  }
  void get_aux(double* a) const override { hostconv::get_aux<BLK>(d.data(), f.data(), ii.data(), N, a); }
  void set_aux(const double* a) override { hostconv::set_aux<BLK>(d.data(), f.data(), ii.data(), N, a); }
  void get_xpose(double* xq, double* xp) const override { hostconv::get_xpose<BLK>(d.data(), N, xq, xp); }
  void set_xpose(const double* xq, const double* xp) override { hostconv::set_xpose<BLK>(d.data(), N, xq, xp); }
  void open_stream(Stream<R>& rng, ES& S, size_t i) {
    rng.open(P.seed, P.gid_base + (int64_t)i, S.rng_ctr);
    if (!scripts[i].empty()) { rng.script = scripts[i].data(); rng.script_n = (int)scripts[i].size(); rng.script_pos = spos[i]; }
  }
  void close_stream(Stream<R>& rng, ES& S, size_t i) { S.rng_ctr = rng.ctr; spos[i] = rng.script_pos; }
  void physics(const double* ctrl, int nsub) override {
#pragma omp parallel for schedule(dynamic, 4)
    for (size_t i = 0; i < N; i++) {
      R buf[LDS_WORDS_ENV03];
      Store<R> st{buf, 1};
      physics_mem<R, BLK, R>(P, st, d.data(), f.data(), ii.data(), N, i, (CtrlT<R>)ctrl[2 * i], (CtrlT<R>)ctrl[2 * i + 1], nsub);
    }
  }
  void reset(const uint8_t* mask, float* obs) override {
    for (size_t i = 0; i < N; i++) {
      if (mask && !mask[i]) continue;
      ES S;
      load_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
      Stream<R> rng;
      open_stream(rng, S, i);
      Sim<R, BLK>::env_reset(P, S, rng, obs + 6 * i);
      close_stream(rng, S, i);
      store_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
    }
  }
  void step(const float* act, float* obs, float* rew, uint8_t* term, uint8_t* trunc, float* tobs) override {
#pragma omp parallel for schedule(dynamic, 4)
    for (size_t i = 0; i < N; i++) {
      R buf[LDS_WORDS_ENV03];
      Stream<R> rng;
      rng.open(P.seed, P.gid_base + (int64_t)i, 0u);
      if (!scripts[i].empty()) { rng.script = scripts[i].data(); rng.script_n = (int)scripts[i].size(); rng.script_pos = spos[i]; }
      Store<R> st{buf, 1};
      int te, tr;
      float tob[6];
      if (isnan_(act[2 * i]) | isnan_(act[2 * i + 1])) ii[L::I_BAD * N + i] |= BAD_START_BIT;  // as the step kernel does (brs_kernels.hip: step_body)
      env_step_mem<R, BLK, R>(P, st, rng, d.data(), f.data(), ii.data(), N, i, act[2 * i], act[2 * i + 1], obs + 6 * i, tob, rew[i], te, tr);
      spos[i] = rng.script_pos;
      term[i] = (uint8_t)te; trunc[i] = (uint8_t)tr;
      if (tobs) memcpy(tobs + 6 * i, tob, sizeof tob);
    }
  }
  // physics replaced by a scripted post-step state, exactly like tools/gen_golden.py's stubbed mj_step
  void step_stub(int env, const float* act, const double* qpos, const double* qvel, const double* xquat, const double* xpos,
                 float* obs, float* rew, uint8_t* term, uint8_t* trunc, double* ctrl) override {
    size_t i = env;
    ES S;
    load_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
    Stream<R> rng;
    open_stream(rng, S, i);
    CtrlT<R> cl, cr;
    R r = Sim<R, BLK>::env_pre(P, S, rng, act[0], act[1], cl, cr);
    ctrl[0] = (double)cl; ctrl[1] = (double)cr;
    close_stream(rng, S, i);
    store_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
    // install the post state (row i only) through the same conversion the C ABI uses
    std::vector<double> qp((size_t)L::NQ * N), qv((size_t)L::NV * N), tm(N);
    hostconv::get_state<BLK>(d.data(), f.data(), N, qp.data(), qv.data(), nullptr, tm.data());
    for (int k = 0; k < L::NQ; k++) qp[i * L::NQ + k] = qpos[k];
    for (int k = 0; k < L::NV; k++) qv[i * L::NV + k] = qvel[k];
    for (int k = 0; k < P.nsub; k++) tm[i] += P.h_d;
    std::vector<double> xq(4 * N), xp(3 * N);
    hostconv::get_xpose<BLK>(d.data(), N, xq.data(), xp.data());
    // note: set_state normalises quaternions; the block orientation golden is compared sign/scale-insensitively
    std::vector<double> dsave = d;
    hostconv::set_state<BLK>(d.data(), f.data(), N, qp.data(), qv.data(), nullptr, tm.data());
    for (size_t e = 0; e < N; e++) if (e != i) { for (int k = 0; k < 4; k++) xq[4 * e + k] = dsave[(L::D_XQ + k) * N + e]; for (int k = 0; k < 3; k++) xp[3 * e + k] = dsave[(L::D_XP + k) * N + e]; }
    for (int k = 0; k < 4; k++) xq[4 * i + k] = xquat[k];
    for (int k = 0; k < 3; k++) xp[3 * i + k] = xpos[k];
    hostconv::set_xpose<BLK>(d.data(), N, xq.data(), xp.data());
    load_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
    open_stream(rng, S, i);
    int te, tr;
    float tob[6];
    Sim<R, BLK>::env_post(P, S, rng, r, obs, tob, *rew, te, tr);
    *term = (uint8_t)te; *trunc = (uint8_t)tr;
    close_stream(rng, S, i);
    store_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
  }
  void script(int env, const double* u, int n) override { scripts[env].assign(u, u + n); spos[env] = 0; }
  int script_remaining(int env) const override { return (int)scripts[env].size() - spos[env]; }
  // brs_state.hpp: cost_class on the state as it is stored (what the step kernel leaves as the env's key for its next step);
  // cmp [N][6]: (lhs, rhs) of the floor, wheel and far comparisons
  void cost_class(int* key, double* cmp) const override {
    for (size_t i = 0; i < N; i++) {
      ES S;
      load_state<R, BLK>(S, d.data(), f.data(), ii.data(), N, i);
      R c[6] = {0, 0, 0, 0, 0, 0};
      key[i] = brs::cost_class<R, BLK>(P, S, c);
      for (int k = 0; k < 6; k++) cmp[6 * i + k] = (double)c[k];
    }
  }
};

extern "C" {
void* hs_create(int variant, int n, int use_double, uint64_t seed, int64_t gid_base, int auto_reset, int noise,
                int max_steps, int nsub, double h) {
  bool blk = variant == 2 || variant == 3;
  if (use_double) {
    if (blk) return new HostSim<double, true>(variant, n, seed, gid_base, auto_reset, noise, max_steps, nsub, h);
    return new HostSim<double, false>(variant, n, seed, gid_base, auto_reset, noise, max_steps, nsub, h);
  }
  if (blk) return new HostSim<float, true>(variant, n, seed, gid_base, auto_reset, noise, max_steps, nsub, h);
  return new HostSim<float, false>(variant, n, seed, gid_base, auto_reset, noise, max_steps, nsub, h);
}
void hs_destroy(void* h) { delete (IHost*)h; }
void hs_set_threads(int n) { omp_set_num_threads(n > 0 ? n : 1); }
int hs_nq(void* h) { return ((IHost*)h)->nq(); }
int hs_nv(void* h) { return ((IHost*)h)->nv(); }
void hs_set_state(void* h, const double* a, const double* b, const double* c, const double* d) { ((IHost*)h)->set_state(a, b, c, d); }
void hs_get_state(void* h, double* a, double* b, double* c, double* d) { ((IHost*)h)->get_state(a, b, c, d); }
void hs_get_aux(void* h, double* a) { ((IHost*)h)->get_aux(a); }
void hs_set_aux(void* h, const double* a) { ((IHost*)h)->set_aux(a); }
void hs_get_xpose(void* h, double* a, double* b) { ((IHost*)h)->get_xpose(a, b); }
void hs_set_xpose(void* h, const double* a, const double* b) { ((IHost*)h)->set_xpose(a, b); }
void hs_physics(void* h, const double* ctrl, int nsub) { ((IHost*)h)->physics(ctrl, nsub); }
void hs_reset(void* h, const uint8_t* m, float* obs) { ((IHost*)h)->reset(m, obs); }
void hs_step(void* h, const float* a, float* o, float* r, uint8_t* te, uint8_t* tr, float* to) { ((IHost*)h)->step(a, o, r, te, tr, to); }
void hs_step_stub(void* h, int e, const float* a, const double* qp, const double* qv, const double* xq, const double* xp, float* o, float* r,
                  uint8_t* te, uint8_t* tr, double* ctrl) { ((IHost*)h)->step_stub(e, a, qp, qv, xq, xp, o, r, te, tr, ctrl); }
void hs_script(void* h, int e, const double* u, int n) { ((IHost*)h)->script(e, u, n); }
int hs_script_remaining(void* h, int e) { return ((IHost*)h)->script_remaining(e); }
void hs_cost_class(void* h, int* key, double* cmp) { ((IHost*)h)->cost_class(key, cmp); }
// the kernel source's get_pitch / get_yaw core on one accessor quaternion (float or double instantiation)
void hs_pitch_yaw(const double* xq, int use_double, double* pitch, double* yaw) {
  if (use_double) { double p, y; Sim<double, false>::pitch_yaw(xq, p, y); *pitch = p; *yaw = y; }
  else { float p, y; Sim<float, false>::pitch_yaw(xq, p, y); *pitch = p; *yaw = y; }
}
}
