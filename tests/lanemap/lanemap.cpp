// host build of the lane map's slot arithmetic (balance_robot_mujoco_rl_amd/csrc/brs_state.hpp: lane_slot), for CPU tests
// only: tests/test_lane_map_cpu.py compiles it with g++ into a temporary directory, with and without a -DBRS_RARE_CAP
#include "brs_state.hpp"

using namespace brs;

extern "C" {

int lm_nbucket(void) { return LM_NBUCKET; }
int lm_far(void) { return LM_FAR; }
int lm_rare_cap(void) { return LM_RARE_CAP; }
int lm_bucket_order(int o) { return lm_bucket_at(o); }

// slot of every env: envs are numbered bucket by bucket (cnt[0] envs of bucket 0, then bucket 1, ...), rank = order inside;
// cap: wheel lanes per wave (0: the compiled LM_RARE_CAP)
void lm_slots(const unsigned* cnt, unsigned* slot, unsigned cap) {
  unsigned e = 0;
  for (int b = 0; b < LM_NBUCKET; b++)
    for (unsigned r = 0; r < cnt[b]; r++) slot[e++] = cap ? lane_slot(b, r, cnt, cap) : lane_slot(b, r, cnt);
}

}  // extern "C"
