// rela/screen_env.h -- OPTIONAL extension of the env plug-in boundary (not in the reference's rela/env.h), built like
// rela/frame_row_env.h, for envs that render RAW screens (an ALE-backed env: ALEInterface::getScreenRGB).
//
// The reference's env turns every screen into its observation on the CPU (GameState::computeFeature,
// atari/game_state.h:53-82,122-133: max of the last two screens, bilinear to 84x84, gray, four-plane deque).  An env
// deriving from rela::ScreenEnv hands VectorEnv the two screens instead, and the actor shard computes the feature and
// completes the frame stack on the GPU (include/rela_amd.h: rela_atari_features, rela_*_actor_screens_to_stacks).
//
// Contract: after every reset() and step(), the bound row holds the two screens whose element-wise max is the frame
// computeFeature would push -- screen 0 the current, screen 1 the previous one, [H][W][3] u8 RGB each.  A reset() is a
// restart: the stack becomes that frame four times; a step() slides it by one plane.  obs["s"] must still be a
// [4,84,84] u8 tensor, but in screen mode its content is not read and VectorEnv does not copy it.
//
// Indexed colour: ALE's own screen (ALEInterface::getScreen) is ONE palette index per pixel, and getScreenRGB triples it
// on the host through a 256-entry table.  An env whose screenChannels() is 1 hands over the indices, [H][W] u8 per screen,
// and its table once (screenPalette()); the lookup happens in the feature kernel (rela_atari_features_indexed), a third
// of the bytes cross the link, and the features are those of the expanded screens bit for bit.
//
// VectorEnv uses screen mode only when EVERY env of it is a ScreenEnv of the same shape and format (a mix, differing
// shapes or channel counts, an indexed env without a palette, or an env that is also a FrameRowEnv throw at the first
// reset()); its batch then carries "__screens" ([K][2][H][W][3] u8, indexed: [K][2][H][W] u8, page-locked),
// "__stack_restart" (u8[K]: 1 = the row was just reset) and, indexed, "__palette" ([K][256][3] u8, page-locked: one
// table per row).  Envs without this extension keep working through the paths they use today.
#pragma once
#include <cstdint>

namespace rela {

class ScreenEnv {
 public:
  virtual ~ScreenEnv() = default;
  // `row` = 2*H*W*screenChannels() page-locked bytes that stay valid for the VectorEnv's lifetime.  VectorEnv binds it once, after
  // the env's first reset(): the env copies the pair it holds into the row, and from then on writes its pair there.
  virtual void bindScreenRow(uint8_t* row) = 0;
  virtual int screenHeight() const = 0;
  virtual int screenWidth() const = 0;
  // 3 = RGB-interleaved screens (the default), 1 = palette indices
  virtual int screenChannels() const { return 3; }
  // indexed screens: 768 bytes, [256][3] u8 RGB, fixed from the env's first reset() on (VectorEnv reads them once, when
  // it binds the row); every index 0..255 may occur on a screen.  RGB screens: nullptr.
  virtual const uint8_t* screenPalette() const { return nullptr; }
};

}  // namespace rela
