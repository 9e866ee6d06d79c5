// dedup_refs.h -- the references of a de-duplicated frame stack.  Per env-step an actor shard stores the
// stack it acted on in the replay's unit ring once and keeps [rows][ups] int32 references to it; the one caller is
// shard_dedup_store (csrc/actor_shard.h), which serves the Ape-X and the R2D2 shard.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rela_amd {
namespace {
// references of the stack just acted on (history slot `cur`), per row:
//   ups == 1            : the stack's own unit
//   ups == 4, keyframe  : its four planes (stored together)
//   ups == 4, otherwise : an episode start repeats the new plane four times (GameState::computeFeature,
//                         atari/game_state.h:66-70); any other step slides the previous stack by one plane (:71-74)
__global__ void dedup_make_refs(int32_t* __restrict__ cur, const int32_t* __restrict__ prev,
                                const uint8_t* __restrict__ prev_term, int R, int ups, int keyframe, int32_t first_idx,
                                int64_t cap) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= R) return;
  if (ups == 1) {
    cur[row] = (int32_t)(((int64_t)first_idx + row) % cap);
    return;
  }
  int32_t* c = cur + (size_t)row * 4;
  if (keyframe) {
    for (int k = 0; k < 4; ++k) c[k] = (int32_t)(((int64_t)first_idx + 4 * row + k) % cap);
    return;
  }
  const int32_t fresh = (int32_t)(((int64_t)first_idx + row) % cap);
  if (prev_term[row]) {
    c[0] = c[1] = c[2] = c[3] = fresh;
  } else {
    const int32_t* p = prev + (size_t)row * 4;
    c[0] = p[1], c[1] = p[2], c[2] = p[3], c[3] = fresh;
  }
}

}  // namespace
}  // namespace rela_amd
