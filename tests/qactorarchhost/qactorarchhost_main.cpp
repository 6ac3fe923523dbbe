// A program of its own around the host build of the int8 off-policy actor (brs_qactor.hpp) at the widths of one instantiation
// (-DQAH_WIDTHS=Widths256, the default, or WidthsReference), so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_qactor_arch_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and compares what the two print).
//
//   qactorarchhost_main CASE...   each CASE a file written by the test: int32 n; double input_scale, action_scale; int32
//                                 input_zero, action_zero; per layer (6/H0, H0/H1, H1/2): double out_scale; int32 out_zero; int8
//                                 W[out][in]; int32 b[out]; double bias_scale[out]; then int8 table[256]; float obs[n][6]
// For every case: build_image, act_env on every row; one line with n and FNV-1a digests of the actions and of the codes.
#include <inttypes.h>
#include <stdio.h>

#include <memory>
#include <vector>

#include "brs_qactor.hpp"

#ifndef QAH_WIDTHS
#define QAH_WIDTHS Widths256
#endif

namespace {

using Widths = brs::qactor::QAH_WIDTHS;
using Image = brs::qactor::ImageT<Widths>;

uint64_t fnv(const void* data, size_t bytes) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

template <class T> bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  using brs::qactor::OBS, brs::qactor::ACT, brs::qactor::build_image, brs::qactor::act_env;
  static const int NIN[3] = {OBS, Widths::H0, Widths::H1}, NOUT[3] = {Widths::H0, Widths::H1, ACT};
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t n = 0, zeros[2];
    double scales[2];
    if (!f || fread(&n, sizeof(n), 1, f) != 1 || n <= 0 || fread(scales, sizeof(double), 2, f) != 2 || fread(zeros, sizeof(int32_t), 2, f) != 2) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    brs_qactor_model model = {};
    model.input_scale = scales[0]; model.action_scale = scales[1];
    model.input_zero = zeros[0]; model.action_zero = zeros[1];
    std::vector<int8_t> W[3], table;
    std::vector<int32_t> b[3];
    std::vector<double> bs[3];
    std::vector<float> obs;
    bool ok = true;
    for (int k = 0; k < 3 && ok; k++) {
      brs_qlayer& L = model.layer[k];
      L.n_in = NIN[k]; L.n_out = NOUT[k];
      ok = fread(&L.out_scale, sizeof(double), 1, f) == 1 && fread(&L.out_zero, sizeof(int32_t), 1, f) == 1 &&
           read(f, W[k], (size_t)NIN[k] * NOUT[k]) && read(f, b[k], (size_t)NOUT[k]) && read(f, bs[k], (size_t)NOUT[k]);
      L.weight = W[k].data(); L.bias = b[k].data(); L.bias_scale = bs[k].data();
    }
    ok = ok && read(f, table, 256) && read(f, obs, (size_t)n * OBS);
    if (!ok) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    fclose(f);
    model.layer[2].tanh_table = table.data();
    const std::unique_ptr<Image> im(new Image);
    std::string why;
    if (build_image(&model, im.get(), &why) != BRS_OK) {
      fprintf(stderr, "%s: %s\n", argv[a], why.c_str());
      return 2;
    }
    std::vector<float> action((size_t)n * ACT);
    std::vector<int8_t> codes((size_t)n * ACT);
    for (int i = 0; i < n; i++) act_env(*im, &obs[(size_t)OBS * i], &action[(size_t)ACT * i], &codes[(size_t)ACT * i]);
    printf("n=%d action=%016" PRIx64 " codes=%016" PRIx64 "\n", n, fnv(action.data(), action.size() * sizeof(float)), fnv(codes.data(), codes.size()));
  }
  return 0;
}
