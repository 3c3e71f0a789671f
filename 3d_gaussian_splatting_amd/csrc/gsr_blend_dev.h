// gsr_blend_dev.h -- what every kernel that walks a tile's sorted list the way F6 does must share
// with F6: the tile geometry, the workgroup -> tile map, and the alpha of one (pixel, record) pair.
// F6 and B1 (gsr_blend.hip) and the score replay (gsr_scores.hip) compile this one text, under the
// same per-file flags (_build.py: -ffp-contract=off), so the set of contributing pairs and every
// pixel's transmittance are the forward's bit for bit in all three.
#pragma once
#include "gsr_kernels.h"

namespace gsr {

constexpr int kPPL = 4;  // pixels per lane

__device__ inline int xcd_tile(int b, int nwg) {
    // bijective remap: the blocks one XCD receives (b % 8 equal) -> a contiguous tile range
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = b % 8, local = b / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

struct BlendGeom {
    int W, H, grid_x, ty0, nwg;
    // views mode (gsr_forward_views): the image is V views stacked as bands of vgy tile rows;
    // a tile's pixel y is taken relative to its view's band (records are in view coordinates)
    // and rows at or past vh inside a band are padding.  One image: vgy = all rows, vh = H.
    int vgy, vh;
    uint32_t ck_slots;  // checkpoint slots (gsr_internal.h); the live bytes follow the float4 slots
    int ck_fixed;       // 1: slot = tile * 31 + chunk - 1; 0: from the tile's start in the list
    float bg0, bg1, bg2;
    uint32_t cap;       // the binning's capacity: B1 writes partial entries j < cap only
};

// alpha of one (pixel, record) pair, with the reference's two rejections folded into the
// select: power > 0 (here: exponent above log2 o) and alpha < 1/255 give 0.
__device__ __forceinline__ float pair_alpha(float e, float L, float& oG) {
    oG = __builtin_amdgcn_exp2f(e);
    const float a = __builtin_amdgcn_fmed3f(oG, 0.0f, 0.99f);  // = min(0.99, oG): oG >= 0
    return (e <= L && oG >= (1.0f / 255.0f)) ? a : 0.0f;
}

// Same alpha, plus the keep predicate itself: keep implies alpha >= 1/255 > 0 and !keep gives
// alpha = 0, so B1 tests `keep` (an SGPR mask it already has) instead of re-comparing alpha > 0.
__device__ __forceinline__ float pair_alpha_keep(float e, float L, float& oG, bool& keep) {
    oG = __builtin_amdgcn_exp2f(e);
    keep = e <= L && oG >= (1.0f / 255.0f);
    return keep ? __builtin_amdgcn_fmed3f(oG, 0.0f, 0.99f) : 0.0f;
}

// Waves per F6 tile: 2 for a full image (wave w owns stripes 2w, 2w + 1), 4 when the launch
// has too few tiles to fill the chip (multi-GPU bands).  Measured at 1M/1080p with the
// branchless stripe pair: 2 waves 0.258 ms, 1 wave 0.269 (with branches) / 0.343 (branchless,
// 4 stripes), 4 waves 0.299.
constexpr int kF6FullWaves = 2, kF6BandWaves = 4, kF6BandTiles = 4096;

inline BlendGeom make_geo(const gsr_camera& cam, const float bg[3], int ty0, int ty1, long long cap, int vgy, int vh) {
    BlendGeom g;
    g.W = cam.width;
    g.H = cam.height;
    g.vgy = vgy > 0 ? vgy : div_up(cam.height, kTile);
    g.vh = vgy > 0 ? vh : cam.height;
    g.grid_x = div_up(cam.width, kTile);
    g.ty0 = ty0;
    g.nwg = (ty1 - ty0) * g.grid_x;
    const long long full_tiles = (long long)div_up(cam.height, kTile) * g.grid_x;
    g.ck_slots = (uint32_t)ck_pool_slots(cap, full_tiles);  // = BinLayout's
    g.ck_fixed = ck_fixed_layout(cap, full_tiles) ? 1 : 0;
    g.bg0 = bg[0];
    g.bg1 = bg[1];
    g.bg2 = bg[2];
    g.cap = cap > 0 ? (uint32_t)cap : 0u;
    return g;
}

// The tile count a pass picks its instantiation by (and with it the B1 chunk work): the tiles of
// ONE image, so views mode chunks every tile as a per-view call does, which keeps its gradients
// bit-identical.  The aux channel has no say in it (same batches, same chunk quota): a forward's
// chunk table -- and with it every colour gradient bit -- does not depend on whether it rides along.
inline long long image_tiles(const BlendGeom& geo, int vgy) {
    return vgy > 0 ? (long long)geo.vgy * geo.grid_x : geo.nwg;
}

}  // namespace gsr
