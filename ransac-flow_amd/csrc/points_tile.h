// points_tile.h -- the tiling both point-compaction units share: points.hip (N maps of one size) and points_ragged.hip (B maps of
// different sizes, one table row each).  A tile is POINTS_TILE consecutive pixels of ONE map, looked at in POINTS_PASSES passes of
// POINTS_BLOCK threads.
#pragma once
#include <cstddef>

namespace {

constexpr int POINTS_BLOCK = 256;                // 4 wavefronts
constexpr int POINTS_PASSES = 4;
constexpr int POINTS_TILE = POINTS_BLOCK * POINTS_PASSES;
constexpr int POINTS_WAVES = POINTS_BLOCK / 64;
constexpr int POINTS_GRID_CAP = 8192;            // workgroups stride over the tiles beyond it
constexpr int POINTS_SCAN_BLOCK = 1024;          // 16 wavefronts

typedef long long i64x2 __attribute__((ext_vector_type(2)));

inline bool points_aligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

}  // namespace
