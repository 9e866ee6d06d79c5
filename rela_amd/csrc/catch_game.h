// catch_game.h -- Catch on 84x84 in integer arithmetic, the one definition of the game that the device env
// (catch_env.hip), the host env (pybind/synth_atari.cc: CatchEnv) and the CPU shim of the tests compile.
//
// A 4x4 ball falls 4 pixels per step and drifts sideways by dx in {-4, 0, 4}, bouncing off the walls; a 12x3 paddle at
// the bottom moves left, stays or moves right (action % 3 - 1, 4 pixels).  When the ball reaches the paddle's line the
// step pays +1 (caught) or -1 (missed) and a new ball spawns; an episode lasts episode_len steps.  The observation is
// the frame stack of the last four (px, bx, by) triples, plane 3 the newest: it slides by exactly one plane per step
// and a reset repeats the first frame four times, as GameState::computeFeature stacks (atari/game_state.h:53-82).
// The drift is only readable from the stack.  Everything is int32 / uint32, so host and device agree bit for bit.
// Plain C++ apart from the HIP qualifiers: no HIP include, g++ compiles it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RELA_CATCH_HD __host__ __device__
#else
#define RELA_CATCH_HD
#endif

namespace catch_game {

constexpr int kSide = 84;                  // the frame is kSide x kSide
constexpr int kPlane = kSide * kSide;      // bytes of one plane
constexpr int kObs = 4 * kPlane;           // bytes of one observation
constexpr int kCell = 4;                   // ball side, and the step of every movement
constexpr int kBallMaxX = kSide - kCell;   // 80: the ball's bx lies in 0..80
constexpr int kPaddleW = 12, kPaddleY = 80, kPaddleH = 3;
constexpr int kPaddleMaxX = kSide - kPaddleW;  // 72
constexpr int kLine = 80;                  // a ball with by >= kLine has landed
constexpr uint8_t kBallPixel = 255, kPaddlePixel = 170;

struct Frame {  // what one plane is drawn from
  int32_t px, bx, by;
};

// the paddle's move of an action id: ids alias onto left / stay / right
RELA_CATCH_HD inline int move_of(int64_t action) { return (int)(action % 3) - 1; }

// pixel (y, x) of the plane of one history entry
RELA_CATCH_HD inline uint8_t pixel(const Frame& f, int y, int x) {
  if (y >= f.by && y < f.by + kCell && x >= f.bx && x < f.bx + kCell) return kBallPixel;
  if (y >= kPaddleY && y < kPaddleY + kPaddleH && x >= f.px && x < f.px + kPaddleW) return kPaddlePixel;
  return 0;
}

// The same picture four pixels at a time.  px and bx are always multiples of kCell = 4 (spawn and reset draw multiples,
// every move is +-4, a reflection maps a multiple onto a multiple) and so is the row pitch, so the ball's four pixels of a
// row are ONE aligned 32-bit word of the plane and the paddle's twelve are three: word `c` (0..20) of pixel row `y`.
constexpr int kWordsPerRow = kSide / 4;
static_assert(kSide % 4 == 0 && kCell == 4 && kPaddleW % 4 == 0, "pixel_word: four pixels of one kind per aligned word");
RELA_CATCH_HD inline uint32_t pixel_word(const Frame& f, int y, int c) {
  if (y >= f.by && y < f.by + kCell && 4 * c == f.bx) return 0x01010101u * kBallPixel;
  if (y >= kPaddleY && y < kPaddleY + kPaddleH && 4 * c >= f.px && 4 * c < f.px + kPaddleW) return 0x01010101u * kPaddlePixel;
  return 0;
}

struct Game {
  uint32_t lcg;
  int32_t px, bx, by, dx, steps, ep_return;
  Frame hist[4];  // hist[3] is the newest

  RELA_CATCH_HD void seed(int64_t s) { lcg = (uint32_t)s * 2654435761u + 40503u; }
  RELA_CATCH_HD uint32_t next() {
    lcg = lcg * 1664525u + 1013904223u;
    return lcg;
  }
  RELA_CATCH_HD void spawn() {
    bx = kCell * (int32_t)((next() >> 24) % 21u);
    dx = kCell * ((int32_t)((next() >> 24) % 3u) - 1);
    by = 0;
  }
  RELA_CATCH_HD void reset() {
    steps = 0;
    ep_return = 0;
    px = kCell * (int32_t)((next() >> 24) % 19u);
    spawn();
    const Frame f = {px, bx, by};
    hist[0] = hist[1] = hist[2] = hist[3] = f;
  }
  // one step with the paddle's move in {-1, 0, 1}; -> the reward (-1, 0, +1); *terminal: the episode is over
  RELA_CATCH_HD int32_t step(int move, int episode_len, bool* terminal) {
    px += kCell * move;
    px = px < 0 ? 0 : (px > kPaddleMaxX ? kPaddleMaxX : px);
    bx += dx;
    if (bx < 0) {
      bx = -bx;
      dx = -dx;
    }
    if (bx > kBallMaxX) {
      bx = 2 * kBallMaxX - bx;
      dx = -dx;
    }
    by += kCell;
    int32_t reward = 0;
    if (by >= kLine) {
      reward = (bx + kCell - 1 >= px && bx <= px + kPaddleW - 1) ? 1 : -1;
      spawn();
    }
    hist[0] = hist[1];
    hist[1] = hist[2];
    hist[2] = hist[3];
    const Frame f = {px, bx, by};
    hist[3] = f;
    ++steps;
    ep_return += reward;
    *terminal = steps >= episode_len;
    return reward;
  }
};

// VectorEnv::reset followed by act: a step whose episode ends reports terminal with the step's reward, hands the finished
// episode's return and length to the caller and leaves the game already reset, so the next observation is the first of
// the new episode.  LCG draws in that case: the landing's spawn(), reset()'s px, reset()'s spawn().
RELA_CATCH_HD inline int32_t step_autoreset(Game& g, int move, int episode_len, bool* terminal, int32_t* done_return,
                                            int32_t* done_len) {
  const int32_t reward = g.step(move, episode_len, terminal);
  if (*terminal) {
    *done_return = g.ep_return;
    *done_len = g.steps;
    g.reset();
  }
  return reward;
}

// host rendering of the four planes: out = [4][84][84] u8
// (the paddle first, the ball over it, as pixel() orders them; every rectangle lies inside the plane)
inline void render(const Game& g, uint8_t* out) {
  for (int i = 0; i < kObs; ++i) out[i] = 0;
  for (int p = 0; p < 4; ++p) {
    const Frame& f = g.hist[p];
    uint8_t* plane = out + p * kPlane;
    for (int y = kPaddleY; y < kPaddleY + kPaddleH; ++y)
      for (int x = f.px; x < f.px + kPaddleW; ++x) plane[y * kSide + x] = kPaddlePixel;
    for (int y = f.by; y < f.by + kCell; ++y)
      for (int x = f.bx; x < f.bx + kCell; ++x) plane[y * kSide + x] = kBallPixel;
  }
}

}  // namespace catch_game
