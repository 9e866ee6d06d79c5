// catch_env.hip -- the device-resident Catch env (rela_catch_*): every row of an actor shard plays one game of
// catch_game.h, its state lives in HBM and its frame stack is rendered straight into the address the caller gives
// (an actor shard's observation slot), so a tick moves no observation, reward or terminal over PCIe.
//
//   catch_step_render   one launch: step every row with its action, re-initialise the rows whose episode ended, write
//                       reward (f32) and terminal (u8), render every row's next stack
//   catch_step          the first half alone (rela_catch_step with obs_dev == null)
//   catch_render        the second half alone (rela_catch_render)
//   catch_reset_render  reset() of every row and its stack (rela_catch_reset)
//
// The two halves exist because an actor shard WITH a replay keeps all n + 1 history slots live during post_step(): the
// slot the next observation goes to still holds obs_t-n of the transition being inserted, and post_step() needs the
// reward first.  Such a caller steps, calls post_step(), then renders.  A shard without a replay (evaluation) acts on
// one slot and takes the fused launch.
//
// Write bound: 28,224 B per row and tick (180.6 MB at 6,400 rows), nothing is read but 20 words of state per row.  One
// block of 256 threads = one row.  Every thread loads the row's state -- the address is uniform over the block, so these
// are scalar loads and the step itself runs on the scalar unit -- and steps the game redundantly; thread 0 alone stores
// the new state, into the OTHER of two state buffers (the host flips them per launch), so no thread can read a word that
// another has already replaced: no atomics, no LDS, no barrier.  Each thread then writes 16-byte units of the stack: a
// unit spans at most two pixel rows, and unless one of them meets the ball's four rows or the paddle's three it is a
// zero store; the others (under 10 %) build their four words with catch_game.h's pixel_word() (px and bx are multiples of
// four, so four pixels of one kind share an aligned word).
#include "catch_game.h"
#include "common.h"
#include "prof.h"

using catch_game::Frame;
using catch_game::Game;
using catch_game::kObs;
using catch_game::kPlane;
using catch_game::kSide;

struct rela_catch {
  int device = 0;
  int rows = 0, num_action = 0, episode_len = 0;
  int32_t* state[2] = {nullptr, nullptr};  // [kFields][rows] each: the launch reads state[cur] and writes state[cur ^ 1]
  int cur = 0;
  int32_t* stats = nullptr;  // [4][rows]: episodes, return_sum, last_return, last_len
};

namespace {

// fields of a state buffer, [field][rows] int32
enum { kLcg = 0, kPx, kBx, kBy, kDx, kSteps, kReturn, kBad, kHist, kFields = kHist + 12 };
constexpr int kThreads = 256;
constexpr int kUnitsPerPlane = kPlane / 16;  // 441 16-byte units
static_assert(kPlane % 16 == 0 && catch_game::kWordsPerRow > 4, "a unit lies in one plane and spans at most two pixel rows");

__device__ inline void load_row(const int32_t* __restrict__ st, int rows, int r, Game& g, int32_t& bad) {
  g.lcg = (uint32_t)st[(size_t)kLcg * rows + r];
  g.px = st[(size_t)kPx * rows + r];
  g.bx = st[(size_t)kBx * rows + r];
  g.by = st[(size_t)kBy * rows + r];
  g.dx = st[(size_t)kDx * rows + r];
  g.steps = st[(size_t)kSteps * rows + r];
  g.ep_return = st[(size_t)kReturn * rows + r];
  bad = st[(size_t)kBad * rows + r];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    g.hist[p].px = st[(size_t)(kHist + 3 * p) * rows + r];
    g.hist[p].bx = st[(size_t)(kHist + 3 * p + 1) * rows + r];
    g.hist[p].by = st[(size_t)(kHist + 3 * p + 2) * rows + r];
  }
}

__device__ inline void store_row(int32_t* __restrict__ st, int rows, int r, const Game& g, int32_t bad) {
  st[(size_t)kLcg * rows + r] = (int32_t)g.lcg;
  st[(size_t)kPx * rows + r] = g.px;
  st[(size_t)kBx * rows + r] = g.bx;
  st[(size_t)kBy * rows + r] = g.by;
  st[(size_t)kDx * rows + r] = g.dx;
  st[(size_t)kSteps * rows + r] = g.steps;
  st[(size_t)kReturn * rows + r] = g.ep_return;
  st[(size_t)kBad * rows + r] = bad;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    st[(size_t)(kHist + 3 * p) * rows + r] = g.hist[p].px;
    st[(size_t)(kHist + 3 * p + 1) * rows + r] = g.hist[p].bx;
    st[(size_t)(kHist + 3 * p + 2) * rows + r] = g.hist[p].by;
  }
}

// What one launch does to a row before rendering.  `writer`: this thread stores the row's outputs.
struct StepArgs {
  const int32_t* in;       // state read
  int32_t* out;            // state written
  int32_t* stats;          // [4][rows]
  const int64_t* action;   // [rows]
  float* reward;           // [rows]
  uint8_t* terminal;       // [rows]
  int rows, num_action, episode_len;
};

__device__ inline void step_row(const StepArgs& k, int r, bool writer, Game& g) {
  int32_t bad;
  load_row(k.in, k.rows, r, g, bad);
  const int64_t a = k.action[r];
  int32_t reward = 0, done_return = 0, done_len = 0;
  bool terminal = false;
  if (a < 0 || a >= k.num_action) {  // not an action: the row stays as it is and counts it
    bad += 1;
  } else {
    reward = catch_game::step_autoreset(g, catch_game::move_of(a), k.episode_len, &terminal, &done_return, &done_len);
  }
  if (!writer) return;
  store_row(k.out, k.rows, r, g, bad);
  k.reward[r] = (float)reward;
  k.terminal[r] = terminal ? 1 : 0;
  if (terminal) {  // the row's own entries: nobody else touches them
    k.stats[r] += 1;
    k.stats[(size_t)k.rows + r] += done_return;
    k.stats[(size_t)2 * k.rows + r] = done_return;
    k.stats[(size_t)3 * k.rows + r] = done_len;
  }
}

// one aligned word of a plane (four pixels), then on to the next word of the plane
__device__ inline uint32_t next_word(const Frame& f, int& y, int& c) {
  const uint32_t w = catch_game::pixel_word(f, y, c);
  if (++c == catch_game::kWordsPerRow) {
    c = 0;
    ++y;
  }
  return w;
}

// the row's stack, [4][84][84] u8 at `dst` (16-byte aligned), by the block's threads
__device__ inline void render_row(const Game& g, uint8_t* __restrict__ dst) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const Frame f = g.hist[p];
    uint4* plane = reinterpret_cast<uint4*>(dst + (size_t)p * kPlane);
    for (int j = threadIdx.x; j < kUnitsPerPlane; j += kThreads) {
      const int w0 = 4 * j;  // the unit's first word
      int y = w0 / catch_game::kWordsPerRow, c = w0 - y * catch_game::kWordsPerRow;
      const int y1 = c + 3 >= catch_game::kWordsPerRow ? y + 1 : y;  // the unit's last pixel row
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      const bool ball = y1 >= f.by && y < f.by + catch_game::kCell;
      const bool paddle = y1 >= catch_game::kPaddleY && y < catch_game::kPaddleY + catch_game::kPaddleH;
      if (ball || paddle) {
        v.x = next_word(f, y, c);
        v.y = next_word(f, y, c);
        v.z = next_word(f, y, c);
        v.w = next_word(f, y, c);
      }
      plane[j] = v;
    }
  }
}

__global__ __launch_bounds__(kThreads) void catch_step_render(const StepArgs k, uint8_t* __restrict__ obs) {
  const int r = blockIdx.x;  // grid = rows
  Game g;
  step_row(k, r, threadIdx.x == 0, g);
  render_row(g, obs + (size_t)r * kObs);
}

__global__ __launch_bounds__(kThreads) void catch_step(const StepArgs k) {
  const int r = blockIdx.x * kThreads + threadIdx.x;  // one thread per row
  if (r >= k.rows) return;
  Game g;
  step_row(k, r, true, g);
}

__global__ __launch_bounds__(kThreads) void catch_render(const int32_t* __restrict__ st, int rows, uint8_t* __restrict__ obs) {
  const int r = blockIdx.x;
  Game g;
  int32_t bad;
  load_row(st, rows, r, g, bad);
  render_row(g, obs + (size_t)r * kObs);
}

__global__ __launch_bounds__(kThreads) void catch_reset_render(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                               int rows, uint8_t* __restrict__ obs) {
  const int r = blockIdx.x;
  Game g;
  int32_t bad;
  load_row(in, rows, r, g, bad);
  g.reset();
  if (threadIdx.x == 0) store_row(out, rows, r, g, bad);
  render_row(g, obs + (size_t)r * kObs);
}

}  // namespace

using namespace rela_amd;

extern "C" int rela_catch_create(rela_catch** out, int rows, int num_action, int episode_len, uint64_t seed, int device) {
  RELA_CHECK(out && rows >= 1 && num_action >= 3 && episode_len >= 1, RELA_EINVAL,
             "rela_catch_create: bad arguments (rows=%d A=%d episode_len=%d; needs rows >= 1, A >= 3, episode_len >= 1)", rows,
             num_action, episode_len);
  int rc = check_device(device, "rela_catch_create");
  if (rc != RELA_OK) return rc;
  DeviceGuard g(device);
  auto* c = new rela_catch();
  c->device = device;
  c->rows = rows;
  c->num_action = num_action;
  c->episode_len = episode_len;
  const size_t words = (size_t)kFields * rows;
  std::vector<int32_t> init(words, 0);  // row r plays the game seeded seed + r; nothing is drawn before the first reset
  for (int r = 0; r < rows; ++r) {
    Game game;
    game.seed((int64_t)(seed + (uint64_t)r));
    init[(size_t)kLcg * rows + r] = (int32_t)game.lcg;
  }
  for (int b = 0; b < 2; ++b) {
    if (hipMalloc(reinterpret_cast<void**>(&c->state[b]), words * sizeof(int32_t)) != hipSuccess ||
        hipMemcpy(c->state[b], init.data(), words * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
      set_last_error("rela_catch_create: state of %d rows: allocation or upload failed", rows);
      rela_catch_destroy(c);
      return RELA_ENOMEM;
    }
  }
  if (hipMalloc(reinterpret_cast<void**>(&c->stats), (size_t)4 * rows * sizeof(int32_t)) != hipSuccess ||
      hipMemset(c->stats, 0, (size_t)4 * rows * sizeof(int32_t)) != hipSuccess) {
    set_last_error("rela_catch_create: statistics of %d rows: allocation failed", rows);
    rela_catch_destroy(c);
    return RELA_ENOMEM;
  }
  *out = c;
  return RELA_OK;
}

extern "C" void rela_catch_destroy(rela_catch* c) {
  if (!c) return;
  DeviceGuard g(c->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(c->state[0]);
  (void)hipFree(c->state[1]);
  (void)hipFree(c->stats);
  delete c;
}

extern "C" int rela_catch_reset(rela_catch* c, uint8_t* obs_dev, void* stream) {
  RELA_CHECK(c && obs_dev && ((uintptr_t)obs_dev & 15) == 0, RELA_EINVAL,
             "rela_catch_reset: bad arguments (the observation buffer must be 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(c->device);
  ProfScope prof("catch_reset_render", s);
  note_launch("catch_reset_render");
  hipLaunchKernelGGL(catch_reset_render, dim3(c->rows), dim3(kThreads), 0, s, c->state[c->cur], c->state[c->cur ^ 1], c->rows,
                     obs_dev);
  RELA_LAUNCH_CHECK();
  c->cur ^= 1;
  return RELA_OK;
}

extern "C" int rela_catch_step(rela_catch* c, const int64_t* action_dev, uint8_t* obs_dev, float* reward_dev,
                               uint8_t* terminal_dev, void* stream) {
  RELA_CHECK(c && action_dev && reward_dev && terminal_dev && ((uintptr_t)obs_dev & 15) == 0, RELA_EINVAL,
             "rela_catch_step: bad arguments (the observation buffer must be 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(c->device);
  const StepArgs k = {c->state[c->cur], c->state[c->cur ^ 1], c->stats, action_dev, reward_dev, terminal_dev,
                      c->rows, c->num_action, c->episode_len};
  if (obs_dev) {
    ProfScope prof("catch_step_render", s);
    note_launch("catch_step_render");
    hipLaunchKernelGGL(catch_step_render, dim3(c->rows), dim3(kThreads), 0, s, k, obs_dev);
  } else {
    ProfScope prof("catch_step", s);
    note_launch("catch_step");
    hipLaunchKernelGGL(catch_step, dim3(ceil_div(c->rows, kThreads)), dim3(kThreads), 0, s, k);
  }
  RELA_LAUNCH_CHECK();
  c->cur ^= 1;
  return RELA_OK;
}

extern "C" int rela_catch_render(rela_catch* c, uint8_t* obs_dev, void* stream) {
  RELA_CHECK(c && obs_dev && ((uintptr_t)obs_dev & 15) == 0, RELA_EINVAL,
             "rela_catch_render: bad arguments (the observation buffer must be 16-byte aligned)");
  hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(c->device);
  ProfScope prof("catch_render", s);
  note_launch("catch_render");
  hipLaunchKernelGGL(catch_render, dim3(c->rows), dim3(kThreads), 0, s, c->state[c->cur], c->rows, obs_dev);
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

extern "C" const int32_t* rela_catch_stats_dev(const rela_catch* c) { return c ? c->stats : nullptr; }

extern "C" int rela_catch_debug_state(rela_catch* c, int32_t* host_dst) {
  RELA_CHECK(c && host_dst, RELA_EINVAL, "rela_catch_debug_state: bad arguments");
  DeviceGuard g(c->device);
  RELA_HIP(hipDeviceSynchronize());
  std::vector<int32_t> st((size_t)8 * c->rows);  // the first eight fields are the ones reported, in their order
  RELA_HIP(hipMemcpy(st.data(), c->state[c->cur], st.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int r = 0; r < c->rows; ++r)
    for (int f = 0; f < 8; ++f) host_dst[(size_t)r * 8 + f] = st[(size_t)f * c->rows + r];
  return RELA_OK;
}
