// Host build of the int8 off-policy actor's kernel source (balance_robot_mujoco_rl_amd/csrc/brs_qactor.hpp) at the widths of one
// instantiation, named at compile time: -DQAH_WIDTHS=Widths256 (the default: 6-256-256-2) or WidthsReference (6-300-200-2).  The
// checks and the zero-point fold of brs_qpolicy_actor_set_model for those widths, and the per-env scalar form of the kernel's
// arithmetic (tests/test_qactor_arch_cpu.py builds this with g++ as a shared object; qactorarchhost_main.cpp is the program the
// sanitizers run).  tests/qactorhost is the same for the names without a template parameter.
#include "brs_qactor.hpp"

#include <string.h>

#ifndef QAH_WIDTHS
#define QAH_WIDTHS Widths256
#endif

namespace {
using Widths = brs::qactor::QAH_WIDTHS;
using Image = brs::qactor::ImageT<Widths>;
}  // namespace

extern "C" {

int qah_image_bytes() { return (int)sizeof(Image); }
int qah_arch() { return Widths::ID; }
void qah_widths(int* h0, int* h1, int* h0p, int* h1p) { *h0 = Widths::H0; *h1 = Widths::H1; *h0p = Widths::H0P; *h1p = Widths::H1P; }

// brs_qpolicy_actor_set_model without the device: 0 and the image, or BRS_ERR_ARG and the reason in err[err_len]
int qah_build(const brs_qactor_model* model, void* image, char* err, int err_len) {
  std::string why;
  const int rc = brs::qactor::build_image(model, (Image*)image, &why);
  if (err && err_len > 0) { strncpy(err, why.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
  return rc;
}

// brs_qpolicy_actor_act on the host: obs[n][6] -> action[n][2], action_q[n][2] (may be NULL)
void qah_act(const void* image, int n, const float* obs, float* action, int8_t* action_q) {
  const Image& im = *(const Image*)image;
  for (int i = 0; i < n; i++)
    brs::qactor::act_env(im, obs + (size_t)brs::qactor::OBS * i, action + (size_t)brs::qactor::ACT * i,
                         action_q ? action_q + (size_t)brs::qactor::ACT * i : nullptr);
}

}  // extern "C"
