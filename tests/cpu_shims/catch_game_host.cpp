// CPU shim: the host build of rela_amd/csrc/catch_game.h (the same source the device env compiles), for
// tests/test_catch_host.py.  TEST INFRASTRUCTURE.
// With -DCATCH_MAIN it is a stand-alone program (random play with every invariant checked) for a host-only sanitizer run:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DCATCH_MAIN catch_game_host.cpp && ./a.out
#include <stddef.h>

#include "../../rela_amd/csrc/catch_game.h"

using catch_game::Game;

static void put_state(const Game& g, int32_t bad, int32_t* s) {
  s[0] = (int32_t)g.lcg;
  s[1] = g.px, s[2] = g.bx, s[3] = g.by, s[4] = g.dx, s[5] = g.steps, s[6] = g.ep_return, s[7] = bad;
}

// One game with the device env's vector semantics (step_autoreset; an action outside [0, num_action) leaves the game as
// it is and counts).  obs: [n + 1][4][84][84], entry 0 the reset observation, entry i + 1 the one after step i;
// state: [n + 1][8] likewise; reward: [n] int32; terminal: [n] u8; stats: [4] episodes, return_sum, last_return, last_len.
extern "C" void shim_catch_run(int64_t seed, int num_action, int episode_len, const int64_t* actions, int n, uint8_t* obs,
                               int32_t* state, int32_t* reward, uint8_t* terminal, int32_t* stats) {
  Game g = Game();
  g.seed(seed);
  g.reset();
  int32_t bad = 0;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  catch_game::render(g, obs);
  put_state(g, bad, state);
  for (int i = 0; i < n; ++i) {
    const int64_t a = actions[i];
    int32_t r = 0, done_return = 0, done_len = 0;
    bool t = false;
    if (a < 0 || a >= num_action) {
      bad += 1;
    } else {
      r = catch_game::step_autoreset(g, catch_game::move_of(a), episode_len, &t, &done_return, &done_len);
    }
    if (t) {
      stats[0] += 1;
      stats[1] += done_return;
      stats[2] = done_return;
      stats[3] = done_len;
    }
    reward[i] = r;
    terminal[i] = t ? 1 : 0;
    catch_game::render(g, obs + (size_t)(i + 1) * catch_game::kObs);
    put_state(g, bad, state + (size_t)(i + 1) * 8);
  }
}

// pixel() over a whole stack, the per-pixel definition the kernel evaluates: out = [4][84][84]
extern "C" void shim_catch_pixels(const int32_t* hist12, uint8_t* out) {
  for (int p = 0; p < 4; ++p) {
    const catch_game::Frame f = {hist12[3 * p], hist12[3 * p + 1], hist12[3 * p + 2]};
    for (int y = 0; y < catch_game::kSide; ++y)
      for (int x = 0; x < catch_game::kSide; ++x) out[(p * catch_game::kSide + y) * catch_game::kSide + x] = catch_game::pixel(f, y, x);
  }
}

// ... and pixel_word(), four pixels at a time, as the kernel stores them: out = [4][84][21] u32
extern "C" void shim_catch_pixel_words(const int32_t* hist12, uint32_t* out) {
  for (int p = 0; p < 4; ++p) {
    const catch_game::Frame f = {hist12[3 * p], hist12[3 * p + 1], hist12[3 * p + 2]};
    for (int y = 0; y < catch_game::kSide; ++y)
      for (int c = 0; c < catch_game::kWordsPerRow; ++c)
        out[(p * catch_game::kSide + y) * catch_game::kWordsPerRow + c] = catch_game::pixel_word(f, y, c);
  }
}

// `episodes` episodes of the policy that walks the paddle towards bx - 4; returns[e] = the episode's return
extern "C" void shim_catch_walk(int64_t seed, int episode_len, int episodes, int32_t* returns) {
  Game g = Game();
  g.seed(seed);
  for (int e = 0; e < episodes; ++e) {
    g.reset();
    bool t = false;
    while (!t) {
      const int target = g.bx - 4;
      const int64_t a = g.px > target ? 0 : (g.px < target ? 2 : 1);
      g.step(catch_game::move_of(a), episode_len, &t);
    }
    returns[e] = g.ep_return;
  }
}

#ifdef CATCH_MAIN
#include <stdio.h>

#include <vector>

int main() {
  const int n = 2000, episode_len = 45, A = 18;
  std::vector<int64_t> actions(n);
  uint32_t x = 12345u;
  for (int i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    actions[i] = (int64_t)((x >> 16) % (A + 2)) - 1;  // -1 .. A: both bad actions occur
  }
  std::vector<uint8_t> obs((size_t)(n + 1) * catch_game::kObs), term(n);
  std::vector<int32_t> state((size_t)(n + 1) * 8), reward(n);
  int32_t stats[4];
  int bad = 0;
  for (int64_t seed = 0; seed < 3; ++seed) {
    shim_catch_run(seed, A, episode_len, actions.data(), n, obs.data(), state.data(), reward.data(), term.data(), stats);
    for (int i = 0; i <= n; ++i) {
      const int32_t* s = &state[(size_t)i * 8];
      if (s[1] < 0 || s[1] > 72 || s[2] < 0 || s[2] > 80 || s[3] < 0 || s[3] > 76 || s[5] < 0 || s[5] >= episode_len) ++bad;
    }
    for (int i = 0; i < n; ++i)
      if (reward[i] < -1 || reward[i] > 1) ++bad;
  }
  int32_t ret[5];
  shim_catch_walk(7, 200, 5, ret);
  for (int e = 0; e < 5; ++e)
    if (ret[e] != 10) ++bad;
  printf("catch_game_host: 3 seeds x %d steps, %d episodes in the last run, walk policy %d, %d violations\n", n, (int)stats[0],
         (int)ret[0], bad);
  return bad ? 1 : 0;
}
#endif
