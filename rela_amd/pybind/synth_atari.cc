// synth_atari.cc -- second native module (`synth_atari`), the counterpart of the reference's
// atari/pybind.cc:12-30: a C++ subclass of rela::Env registered against rela.Env.
//
// ALE and ROMs are not available in this pipeline, so the env is synthetic but
// keeps the observation contract of atari/atari_env.h:83-155: {"s": u8[4,84,84], "eps": f32[1],
// "legal_move": f32[A]}, clipped rewards in {-1,0,1}, fixed episode length.  Frames come from the
// 32-bit LCG of SURVEY 8d (x <- 1664525 x + 1013904223, top byte), so a run is reproducible from
// (seed, actions) alone.
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cstring>
#include <torch/extension.h>
#include <vector>

#include "rela/env.h"
// this repo's optional in-place rendering extension; absent when this file is compiled against the REFERENCE's
// rela/env.h for the oracle (oracle/Makefile: _ref/synth_atari), where the env is a plain three-virtual rela::Env
#if __has_include("rela/frame_row_env.h")
#include "rela/frame_row_env.h"
#define RELA_HAS_FRAME_ROW 1
#define RELA_FRAME_ROW_BASE , public rela::FrameRowEnv
#else
#define RELA_HAS_FRAME_ROW 0
#define RELA_FRAME_ROW_BASE
#endif
// ... and the raw-screen extension with the feature recipe it shares with the kernel (absent in the oracle's build)
#if __has_include("rela/screen_env.h") && __has_include("../csrc/atari_screen.h")
#include "../csrc/atari_screen.h"
#include "rela/screen_env.h"
#define RELA_HAS_SCREEN 1
#else
#define RELA_HAS_SCREEN 0
#endif
// the Catch game, the same header the device env compiles (csrc/catch_env.hip); plain C++, so the oracle's build has it too
#include "../csrc/catch_game.h"

namespace py = pybind11;

namespace {

// n bytes of the LCG stream (x <- 1664525 x + 1013904223, top byte of every state) starting AFTER `state`; returns the
// last state.  The recurrence is a serial dependency chain (~4 cycles per byte: 28,224 bytes = 37-40 us per frame
// stack, which bounded the threaded benchmark at ~430 k env-steps/s on 16 cores), so 32 consecutive states are carried
// in four 8-lane vectors and advanced by the 32-step jump x_{k+32} = A32 x_k + C32: the same bytes in the same order,
// bit for bit (6 us per frame stack).  Vector k, lane j holds x_{i+4j+k+1}: the top bytes of lane j of the four
// vectors are four CONSECUTIVE output bytes, so the packed word is stored as it is.
typedef uint32_t v8u __attribute__((vector_size(32)));
__attribute__((target_clones("avx2", "default"))) uint32_t lcgFill(uint32_t state, uint8_t* out, int n) {
  constexpr uint32_t a = 1664525u, c = 1013904223u;
  v8u l[4];
  uint32_t A32 = 1, C32 = 0;
  for (int p = 0; p < 32; ++p) {
    state = state * a + c;
    l[p & 3][p >> 2] = state;
    C32 = C32 * a + c;
    A32 *= a;
  }
  int i = 0;
  for (; i + 32 <= n; i += 32) {
    const v8u w = (l[0] >> 24) | ((l[1] >> 24) << 8) | ((l[2] >> 24) << 16) | (l[3] & 0xFF000000u);
    std::memcpy(out + i, &w, 32);
    for (int k = 0; k < 4; ++k) l[k] = l[k] * A32 + C32;
  }
  // l[0][0] is x_{i+1}: the serial tail (n not a multiple of 32) and the returned state continue from
  // x_i = (x_{i+1} - c) * a^-1 (mod 2^32)
  constexpr uint32_t aInv = 4276115653u;  // a * aInv == 1 (mod 2^32)
  uint32_t last = (l[0][0] - c) * aInv;
  for (; i < n; ++i) {
    last = last * a + c;
    out[i] = (uint8_t)(last >> 24);
  }
  return last;
}

class SyntheticAtariEnv : public rela::Env RELA_FRAME_ROW_BASE {
 public:
  // slidingStack: the observation is a stack of four planes of which ONE is new per step and the first plane of
  // an episode is repeated four times -- GameState::computeFeature's stacking (atari/game_state.h:53-82).  The
  // default (false) draws four fresh planes per step, the LCG frames of SURVEY 8d the goldens were recorded with.
  SyntheticAtariEnv(int seed, float eps, int numAction, int episodeLen, bool slidingStack = false)
      : state_((uint32_t)seed), numAction_(numAction), episodeLen_(episodeLen), sliding_(slidingStack), steps_(0),
        terminal_(true), episodeReward_(0.f) {
    eps_ = torch::full({1}, eps, torch::kFloat32);  // shape [1]: SURVEY H6
    legal_ = torch::ones({numAction}, torch::kFloat32);
    frame_ = torch::zeros({4, 84, 84}, torch::kUInt8);
  }

  int numAction() const { return numAction_; }
  float getEpisodeReward() const { return episodeReward_; }

  rela::TensorDict reset() final {
    steps_ = 0;
    terminal_ = false;
    episodeReward_ = 0.f;
    fillFrame(true);
    return observation();
  }

  std::tuple<rela::TensorDict, float, bool> step(const rela::TensorDict& action) final {
    const auto& at = action.at("a");
    const int64_t a = (at.device().is_cpu() && at.scalar_type() == torch::kInt64 && at.numel() == 1)
                          ? *at.data_ptr<int64_t>()  // (item() costs a dispatcher round trip per env-step)
                          : at.item<int64_t>();
    if (a < 0 || a >= numAction_) throw std::out_of_range("SyntheticAtariEnv: action out of range");
    fillFrame(false);
    const uint32_t x = next();
    float reward = 0.f;
    if ((a & 1) == 0) reward = (float)((int)((x >> 24) % 3) - 1);
    episodeReward_ += reward;
    ++steps_;
    if (steps_ >= episodeLen_) terminal_ = true;
    return std::make_tuple(observation(), reward, terminal_);
  }

  bool terminated() const final { return terminal_; }

#if RELA_HAS_FRAME_ROW
  // render into the VectorEnv's page-locked row from now on (it already holds the current observation)
  void bindFrameRow(uint8_t* row) final { frame_ = torch::from_blob(row, {4, 84, 84}, torch::kUInt8); }
  bool slidingStack() const final { return sliding_; }
#endif

 private:
  uint32_t next() {
    state_ = state_ * 1664525u + 1013904223u;
    return state_;
  }
  void fillFrame(bool episodeStart) {
    uint8_t* p = frame_.data_ptr<uint8_t>();
    constexpr int kPlane = 84 * 84;
    if (!sliding_) {
      state_ = lcgFill(state_, p, 4 * kPlane);
      return;
    }
    if (!episodeStart) std::memmove(p, p + kPlane, 3 * kPlane);
    state_ = lcgFill(state_, p + 3 * kPlane, kPlane);
    if (episodeStart)
      for (int k = 0; k < 3; ++k) std::memcpy(p + k * kPlane, p + 3 * kPlane, kPlane);
  }
  rela::TensorDict observation() const { return {{"s", frame_}, {"eps", eps_}, {"legal_move", legal_}}; }

  uint32_t state_;
  const int numAction_, episodeLen_;
  const bool sliding_;
  int steps_;
  bool terminal_;
  float episodeReward_;
  torch::Tensor eps_, legal_, frame_;
};

// Zero-cost env for measuring the ENGINE's own ceiling through rela.Context / BasicThreadLoop / DQNActor (the
// observation is a constant frame stack, the reward 0, episodes end after episode_len steps): whatever rate the
// threaded benchmark reaches with it is what the runtime -- thread loop, VectorEnv, upload, cohort barrier, device
// tick -- can do when the env costs nothing.  The reward is a cheap pseudo-random FLOAT in [-0.5, 0.5): with constant
// frames the Q-values are constant, and constant TD priorities make every float block sum of the replay round the
// same way, so sum_ drifts systematically above the stored weights until a scan runs off the ring -- where the
// reference aborts (prioritized_replay.h:297-302) and this engine raises.
class NullAtariEnv : public rela::Env RELA_FRAME_ROW_BASE {
 public:
  NullAtariEnv(float eps, int numAction, int episodeLen, int seed = 1)
      : numAction_(numAction), episodeLen_(episodeLen), state_((uint32_t)seed * 2654435761u + 12345u) {
    eps_ = torch::full({1}, eps, torch::kFloat32);
    legal_ = torch::ones({numAction}, torch::kFloat32);
    frame_ = torch::full({4, 84, 84}, 17, torch::kUInt8);
  }
  int numAction() const { return numAction_; }
  rela::TensorDict reset() final {
    steps_ = 0;
    terminal_ = false;
    return {{"s", frame_}, {"eps", eps_}, {"legal_move", legal_}};
  }
  std::tuple<rela::TensorDict, float, bool> step(const rela::TensorDict& action) final {
    (void)action;
    if (++steps_ >= episodeLen_) terminal_ = true;
    state_ = state_ * 1664525u + 1013904223u;
    const float reward = (float)(state_ >> 8) * (1.0f / 16777216.0f) - 0.5f;
    return std::make_tuple(rela::TensorDict{{"s", frame_}, {"eps", eps_}, {"legal_move", legal_}}, reward, terminal_);
  }
  bool terminated() const final { return terminal_; }
#if RELA_HAS_FRAME_ROW
  void bindFrameRow(uint8_t* row) final { frame_ = torch::from_blob(row, {4, 84, 84}, torch::kUInt8); }
  bool slidingStack() const final { return true; }  // a constant frame is a stack that slides onto itself
#endif

 private:
  const int numAction_, episodeLen_;
  uint32_t state_;
  int steps_ = 0;
  bool terminal_ = true;
  torch::Tensor eps_, legal_, frame_;
};

// Catch (csrc/catch_game.h): the one env here with something to learn -- a uniformly random policy scores about
// -7 per 200 steps, walking the paddle towards bx - 4 catches every ball (+10).  The host twin of the device env
// (csrc/catch_env.hip: row r of rela_catch_create(seed) is CatchEnv(seed + r)), a plain rela::Env whose stack slides.
class CatchEnv : public rela::Env RELA_FRAME_ROW_BASE {
 public:
  CatchEnv(int seed, float eps, int numAction, int episodeLen) : numAction_(numAction), episodeLen_(episodeLen) {
    if (numAction < 3 || episodeLen < 1) throw std::invalid_argument("CatchEnv: num_action >= 3 and episode_len >= 1");
    game_ = catch_game::Game();
    game_.seed(seed);
    eps_ = torch::full({1}, eps, torch::kFloat32);
    legal_ = torch::ones({numAction}, torch::kFloat32);
    frame_ = torch::zeros({4, 84, 84}, torch::kUInt8);
  }

  int numAction() const { return numAction_; }
  float getEpisodeReward() const { return episodeReward_; }

  rela::TensorDict reset() final {
    terminal_ = false;
    episodeReward_ = 0.f;
    game_.reset();
    catch_game::render(game_, frame_.data_ptr<uint8_t>());
    return observation();
  }

  std::tuple<rela::TensorDict, float, bool> step(const rela::TensorDict& action) final {
    const auto& at = action.at("a");
    const int64_t a = (at.device().is_cpu() && at.scalar_type() == torch::kInt64 && at.numel() == 1)
                          ? *at.data_ptr<int64_t>()
                          : at.item<int64_t>();
    if (a < 0 || a >= numAction_) throw std::out_of_range("CatchEnv: action out of range");
    bool terminal = false;
    const float reward = (float)game_.step(catch_game::move_of(a), episodeLen_, &terminal);
    terminal_ = terminal;
    episodeReward_ += reward;
    catch_game::render(game_, frame_.data_ptr<uint8_t>());
    return std::make_tuple(observation(), reward, terminal_);
  }

  bool terminated() const final { return terminal_; }

  // [8] int32: LCG state bits, px, bx, by, dx, steps, ep_return, 0 -- the columns of rela_catch_debug_state (tests)
  torch::Tensor state() const {
    auto t = torch::zeros({8}, torch::kInt32);
    int32_t* p = t.data_ptr<int32_t>();
    p[0] = (int32_t)game_.lcg;
    p[1] = game_.px, p[2] = game_.bx, p[3] = game_.by, p[4] = game_.dx, p[5] = game_.steps, p[6] = game_.ep_return;
    return t;
  }

#if RELA_HAS_FRAME_ROW
  void bindFrameRow(uint8_t* row) final { frame_ = torch::from_blob(row, {4, 84, 84}, torch::kUInt8); }
  bool slidingStack() const final { return true; }
#endif

 private:
  rela::TensorDict observation() const { return {{"s", frame_}, {"eps", eps_}, {"legal_move", legal_}}; }

  catch_game::Game game_;
  const int numAction_, episodeLen_;
  bool terminal_ = true;
  float episodeReward_ = 0.f;
  torch::Tensor eps_, legal_, frame_;
};

#if RELA_HAS_SCREEN
// Raw-screen env: deterministic 210x160 RGB screens like ALE's (ALEInterface::getScreenRGB) -- a background of 10x10
// blocks in an 8-colour palette drawn from the seed, six blocks recoloured per frame by the LCG, and a 12x16 sprite that
// the actions move -- so Q-values and actions depend on the frames.  Every reset() / step() emits a (current, previous)
// screen pair; the observation is GameState::computeFeature of it (atari/game_state.h:53-82,122-133).  This class
// computes it on the host with the restatement of csrc/atari_screen.h, four-plane deque included (device_features =
// False: a plain rela::Env, the reference's method); SyntheticScreenEnvDevice below hands the pair to the VectorEnv
// instead and the actor shard computes the same stacks on the GPU (rela/screen_env.h).
// indexed = true: the same picture as ALE's own screen format (ALEInterface::getScreen), one palette index per pixel --
// index k < 8 is pal_[k], index 8 + k the sprite colour 255 - pal_[k], every other entry of the 256-entry table is 0 -- so
// the expanded screens equal the RGB env's byte for byte, and rewards, terminals and the LCG stream are the same.
class SyntheticScreenEnv : public rela::Env {
 public:
  static constexpr int kH = 210, kW = 160, kBlock = 10;

  SyntheticScreenEnv(int seed, float eps, int numAction, int episodeLen, bool indexed = false)
      : state_((uint32_t)seed * 2246822519u + 374761393u), numAction_(numAction), episodeLen_(episodeLen), indexed_(indexed),
        ch_(indexed ? 1 : 3), screenBytes_(kH * kW * (indexed ? 1 : 3)), own_(2 * (size_t)screenBytes_), pair_(own_.data()),
        bg_((size_t)screenBytes_) {
    eps_ = torch::full({1}, eps, torch::kFloat32);
    legal_ = torch::ones({numAction}, torch::kFloat32);
    frame_ = torch::zeros({4, 84, 84}, torch::kUInt8);
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < 3; ++c) pal_[k][c] = (uint8_t)(next() >> 24);
    std::memset(table_, 0, sizeof(table_));
    for (int k = 0; k < 8; ++k)
      for (int c = 0; c < 3; ++c) {
        table_[k][c] = pal_[k][c];
        table_[8 + k][c] = (uint8_t)(255 - pal_[k][c]);
      }
    for (int by = 0; by < kH / kBlock; ++by)
      for (int bx = 0; bx < kW / kBlock; ++bx) fillBlock(bg_.data(), by, bx, (int)(next() >> 29));
  }
  ~SyntheticScreenEnv() override = default;

  int numAction() const { return numAction_; }
  float getEpisodeReward() const { return episodeReward_; }

  rela::TensorDict reset() final {
    steps_ = 0;
    terminal_ = false;
    episodeReward_ = 0.f;
    sy_ = (int)((next() >> 24) % (kH - 12));
    sx_ = (int)((next() >> 24) % (kW - 16));
    render(pair_ + screenBytes_);  // the screen before the first one
    render(pair_);
    pushFeature(true);
    return observation();
  }

  std::tuple<rela::TensorDict, float, bool> step(const rela::TensorDict& action) final {
    const auto& at = action.at("a");
    const int64_t a = (at.device().is_cpu() && at.scalar_type() == torch::kInt64 && at.numel() == 1)
                          ? *at.data_ptr<int64_t>()
                          : at.item<int64_t>();
    if (a < 0 || a >= numAction_) throw std::out_of_range("SyntheticScreenEnv: action out of range");
    sx_ = std::min(std::max(sx_ + 4 * ((int)(a % 3) - 1), 0), kW - 16);
    sy_ = std::min(std::max(sy_ + 4 * ((int)((a / 3) % 3) - 1), 0), kH - 12);
    std::memcpy(pair_ + screenBytes_, pair_, screenBytes_);  // the current screen becomes the previous one
    render(pair_);
    pushFeature(false);
    const uint32_t x = next();
    float reward = 0.f;
    if ((a & 1) == 0) reward = (float)((int)((x >> 24) % 3) - 1);
    episodeReward_ += reward;
    ++steps_;
    if (steps_ >= episodeLen_) terminal_ = true;
    return std::make_tuple(observation(), reward, terminal_);
  }

  bool terminated() const final { return terminal_; }

  // the current pair in the env's own format, [2][210][160][3] or, indexed, [2][210][160] (tests)
  torch::Tensor screens() const {
    if (indexed_) return torch::from_blob(pair_, {2, kH, kW}, torch::kUInt8).clone();
    return torch::from_blob(pair_, {2, kH, kW, 3}, torch::kUInt8).clone();
  }
  // the 256-entry RGB table of the indexed format, [256][3] (all the colours the RGB format draws with, too)
  torch::Tensor palette() const { return torch::from_blob((void*)&table_[0][0], {256, 3}, torch::kUInt8).clone(); }

 protected:
  virtual void pushFeature(bool episodeStart) {  // computeFeature's deque, on the host
    constexpr int kPlane = 84 * 84;
    uint8_t* p = frame_.data_ptr<uint8_t>();
    if (!episodeStart) std::memmove(p, p + kPlane, 3 * kPlane);
    if (indexed_) {  // what getScreenRGB does: expand through the table, then the RGB recipe
      rgb_.resize(2 * (size_t)kH * kW * 3);
      for (size_t i = 0; i < 2 * (size_t)screenBytes_; ++i) std::memcpy(&rgb_[3 * i], table_[pair_[i]], 3);
      rela_atari::host_features(rgb_.data(), rgb_.data() + (size_t)kH * kW * 3, kH, kW, p + 3 * kPlane);
    } else {
      rela_atari::host_features(pair_, pair_ + screenBytes_, kH, kW, p + 3 * kPlane);
    }
    if (episodeStart)
      for (int k = 0; k < 3; ++k) std::memcpy(p + k * kPlane, p + 3 * kPlane, kPlane);
  }

  uint32_t state_;
  const int numAction_, episodeLen_;
  const bool indexed_;
  const int ch_;      // bytes per pixel: 3 (RGB) or 1 (palette index)
  const int screenBytes_;  // bytes per screen
  std::vector<uint8_t> own_;
  uint8_t* pair_;  // [2][kH][kW][ch_]: own_, or the VectorEnv's row once bound
  torch::Tensor eps_, legal_, frame_;
  uint8_t table_[256][3];  // the indexed format's RGB table

 private:
  uint32_t next() {
    state_ = state_ * 1664525u + 1013904223u;
    return state_;
  }
  // one pixel in table colour `index` (0..15), as RGB or as the index
  void put(uint8_t* scr, int y, int x, int index) {
    if (indexed_) {
      scr[y * kW + x] = (uint8_t)index;
      return;
    }
    for (int c = 0; c < 3; ++c) scr[(y * kW + x) * 3 + c] = table_[index][c];
  }
  void fillBlock(uint8_t* scr, int by, int bx, int colour) {
    for (int y = by * kBlock; y < (by + 1) * kBlock; ++y)
      for (int x = bx * kBlock; x < (bx + 1) * kBlock; ++x) put(scr, y, x, colour);
  }
  void render(uint8_t* scr) {
    std::memcpy(scr, bg_.data(), screenBytes_);
    for (int k = 0; k < 6; ++k) {
      const uint32_t r = next();
      fillBlock(scr, (int)((r >> 8) % (kH / kBlock)), (int)((r >> 16) % (kW / kBlock)), (int)(r >> 29));
    }
    const int col = 8 + ((steps_ + 3) & 7);  // the sprite: 255 - pal_[...]
    for (int y = sy_; y < sy_ + 12; ++y)
      for (int x = sx_; x < sx_ + 16; ++x) put(scr, y, x, col);
  }
  rela::TensorDict observation() const { return {{"s", frame_}, {"eps", eps_}, {"legal_move", legal_}}; }

  std::vector<uint8_t> bg_, rgb_;
  uint8_t pal_[8][3];
  int steps_ = 0, sy_ = 0, sx_ = 0;
  bool terminal_ = true;
  float episodeReward_ = 0.f;
};

// device_features = True: the same env as a rela::ScreenEnv -- obs["s"] stays a constant [4,84,84] tensor that nobody
// reads, the actor shard builds the stacks from the screen pair in the VectorEnv's row
class SyntheticScreenEnvDevice : public SyntheticScreenEnv, public rela::ScreenEnv {
 public:
  using SyntheticScreenEnv::SyntheticScreenEnv;
  void bindScreenRow(uint8_t* row) final {
    std::memcpy(row, pair_, 2 * (size_t)screenBytes_);
    pair_ = row;
  }
  int screenHeight() const final { return kH; }
  int screenWidth() const final { return kW; }
  int screenChannels() const final { return ch_; }
  const uint8_t* screenPalette() const final { return indexed_ ? &table_[0][0] : nullptr; }

 protected:
  void pushFeature(bool) final {}
};

// synth_atari.screen_features(a, b): the host restatement of csrc/atari_screen.h -- a, b = u8 [H][W][3] (current,
// previous screen) -> u8 [84][84]
// synth_atari.screen_features_indexed(ia, ib, pal): the host restatement for indexed screens -- ia, ib = u8 [H][W]
// palette indices (current, previous screen), pal = u8 [256][3] RGB -> u8 [84][84]
torch::Tensor screenFeaturesIndexed(const torch::Tensor& ia, const torch::Tensor& ib, const torch::Tensor& pal) {
  auto ok = [](const torch::Tensor& t) { return t.scalar_type() == torch::kUInt8 && t.device().is_cpu(); };
  if (ia.dim() != 2 || !ok(ia) || !ok(ib) || !ia.sizes().equals(ib.sizes()))
    throw std::invalid_argument("screen_features_indexed: ia and ib must be uint8 CPU tensors of one shape [H, W]");
  if (!ok(pal) || pal.dim() != 2 || pal.size(0) != 256 || pal.size(1) != 3)
    throw std::invalid_argument("screen_features_indexed: pal must be a uint8 CPU tensor [256, 3]");
  const int H = (int)ia.size(0), W = (int)ia.size(1);
  if (H < rela_atari::kMinIn || H > rela_atari::kMaxIn || W < rela_atari::kMinIn || W > rela_atari::kMaxIn)
    throw std::invalid_argument("screen_features_indexed: screens must be 2..512 x 2..512");
  auto ac = ia.contiguous(), bc = ib.contiguous(), pc = pal.contiguous();
  auto out = torch::empty({84, 84}, torch::kUInt8);
  rela_atari::host_features_indexed(ac.data_ptr<uint8_t>(), bc.data_ptr<uint8_t>(), pc.data_ptr<uint8_t>(), H, W,
                                    out.data_ptr<uint8_t>());
  return out;
}

torch::Tensor screenFeatures(const torch::Tensor& a, const torch::Tensor& b) {
  if (a.dim() != 3 || a.size(2) != 3 || a.scalar_type() != torch::kUInt8 || !a.device().is_cpu() || !a.sizes().equals(b.sizes()) ||
      b.scalar_type() != torch::kUInt8 || !b.device().is_cpu())
    throw std::invalid_argument("screen_features: a and b must be uint8 CPU tensors of one shape [H, W, 3]");
  const int H = (int)a.size(0), W = (int)a.size(1);
  if (H < rela_atari::kMinIn || H > rela_atari::kMaxIn || W < rela_atari::kMinIn || W > rela_atari::kMaxIn)
    throw std::invalid_argument("screen_features: screens must be 2..512 x 2..512");
  auto ac = a.contiguous(), bc = b.contiguous();
  auto out = torch::empty({84, 84}, torch::kUInt8);
  rela_atari::host_features(ac.data_ptr<uint8_t>(), bc.data_ptr<uint8_t>(), H, W, out.data_ptr<uint8_t>());
  return out;
}
#endif

}  // namespace

PYBIND11_MODULE(synth_atari, m) {
  py::module_::import("rela");  // registers the rela.Env base class
  py::class_<SyntheticAtariEnv, rela::Env, std::shared_ptr<SyntheticAtariEnv>>(m, "SyntheticAtariEnv")
      .def(py::init<int, float, int, int, bool>(), py::arg("seed"), py::arg("eps"), py::arg("num_action"),
           py::arg("episode_len"), py::arg("sliding_stack") = false)
      .def("num_action", &SyntheticAtariEnv::numAction)
      .def("reset", &SyntheticAtariEnv::reset)
      .def("step", &SyntheticAtariEnv::step)
      .def("terminated", &SyntheticAtariEnv::terminated)
      .def("get_episode_reward", &SyntheticAtariEnv::getEpisodeReward);
  py::class_<NullAtariEnv, rela::Env, std::shared_ptr<NullAtariEnv>>(m, "NullAtariEnv")
      .def(py::init<float, int, int, int>(), py::arg("eps"), py::arg("num_action"), py::arg("episode_len"), py::arg("seed") = 1)
      .def("num_action", &NullAtariEnv::numAction)
      .def("reset", &NullAtariEnv::reset)
      .def("step", &NullAtariEnv::step)
      .def("terminated", &NullAtariEnv::terminated);
  py::class_<CatchEnv, rela::Env, std::shared_ptr<CatchEnv>>(m, "CatchEnv")
      .def(py::init<int, float, int, int>(), py::arg("seed"), py::arg("eps"), py::arg("num_action"), py::arg("episode_len"))
      .def("num_action", &CatchEnv::numAction)
      .def("reset", &CatchEnv::reset)
      .def("step", &CatchEnv::step)
      .def("terminated", &CatchEnv::terminated)
      .def("get_episode_reward", &CatchEnv::getEpisodeReward)
      .def("state", &CatchEnv::state);
#if RELA_HAS_SCREEN
  py::class_<SyntheticScreenEnv, rela::Env, std::shared_ptr<SyntheticScreenEnv>>(m, "SyntheticScreenEnvHost")
      .def("num_action", &SyntheticScreenEnv::numAction)
      .def("reset", &SyntheticScreenEnv::reset)
      .def("step", &SyntheticScreenEnv::step)
      .def("terminated", &SyntheticScreenEnv::terminated)
      .def("get_episode_reward", &SyntheticScreenEnv::getEpisodeReward)
      .def("screens", &SyntheticScreenEnv::screens)
      .def("palette", &SyntheticScreenEnv::palette);
  py::class_<SyntheticScreenEnvDevice, SyntheticScreenEnv, std::shared_ptr<SyntheticScreenEnvDevice>>(m, "SyntheticScreenEnvDevice");
  m.def("SyntheticScreenEnv",
        [](int seed, float eps, int numAction, int episodeLen, bool deviceFeatures,
           bool indexed) -> std::shared_ptr<SyntheticScreenEnv> {
          if (deviceFeatures) return std::make_shared<SyntheticScreenEnvDevice>(seed, eps, numAction, episodeLen, indexed);
          return std::make_shared<SyntheticScreenEnv>(seed, eps, numAction, episodeLen, indexed);
        },
        py::arg("seed"), py::arg("eps"), py::arg("num_action"), py::arg("episode_len"), py::arg("device_features") = true,
        py::arg("indexed") = false,
        "raw-screen synthetic env: device_features=True -> a rela::ScreenEnv (stacks built on the GPU), False -> a plain "
        "rela::Env that computes the same stacks on the host; indexed=True -> the same picture as palette indices plus a "
        "256-entry table (palette()), False -> RGB screens");
  m.def("screen_features", &screenFeatures, py::arg("a"), py::arg("b"),
        "GameState::computeFeature of one screen pair on the host (csrc/atari_screen.h): u8 [H,W,3] x2 -> u8 [84,84]");
  m.def("screen_features_indexed", &screenFeaturesIndexed, py::arg("ia"), py::arg("ib"), py::arg("pal"),
        "the same from indexed screens (csrc/atari_screen.h: host_features_indexed): u8 [H,W] x2, u8 [256,3] -> u8 [84,84]");
#endif
}
