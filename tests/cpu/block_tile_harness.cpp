// Host build of the tile geometry, plan and index maps of vcf_amd/csrc/vcf_block_tile.h for
// tests/test_block_tile.py: the walks below visit every tile of a frame's plan, the partial
// last one included, element by element in the order of the kernels' loops (scatter_indices,
// gather_indices, crop_pixels), and record where each element goes.  A position outside its
// frame ends a walk with -1.
#include <stdint.h>

#include "vcf_block_tile.h"

using namespace vcf;

// out: Hp, Wp, top, left, nbx, nby, N, TB, LDS class, tiles, moment chunks, staged blocks, LDS bytes
extern "C" void bt_plan(int H, int W, int B, int decode, int elem_bytes, int32_t *out)
{
    const BlockGeom g = make_block_geom(H, W, B);
    const BlockPlan p = make_block_plan(g, decode != 0, elem_bytes);
    const int32_t v[13] = {g.Hp, g.Wp, g.top, g.left, g.nbx, g.nby, g.N, g.TB, p.cls, p.tiles, p.chunks, p.tbm,
                           decode ? dec_lds_bytes(g) : enc_lds_bytes(g, elem_bytes)};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
}

// fn(b, k, c) for every element of every tile, in one of the two orders
template <typename Fn>
static int walk_tiles(const BlockGeom &g, int by_coef, Fn fn)
{
    const BlockPlan p = make_block_plan(g, false, 2);
    for (int t = 0; t < p.tiles; ++t) {
        const int b0 = t * g.TB, tbv = g.TB < g.N - b0 ? g.TB : g.N - b0;
        for (int e = 0; e < tbv * g.D * 3; ++e) {
            int bl, k, c;
            if (by_coef) elem_by_coef(tbv, e, bl, k, c);
            else elem_by_block(g.D, e, bl, k, c);
            if (bl < 0 || bl >= tbv || k < 0 || k >= g.D || c < 0 || c > 2) return -1;
            if (fn(b0 + bl, k, c) < 0) return -1;
        }
    }
    return 0;
}

// scatter_indices: writes[at] counts the stores to byte at of the Hp x Wp x 3 coefficient frame,
// id[at] = (b D + k) 3 + c of the last one
extern "C" int bt_walk_scatter(int H, int W, int B, int sub, int32_t *writes, int32_t *id)
{
    const BlockGeom g = make_block_geom(H, W, B);
    return walk_tiles(g, sub, [&](int b, int k, int c) {
        const long long at = coef_pos(g, b, k, sub) * 3 + c;
        if (at < 0 || at >= g.k_stride) return -1;
        ++writes[at];
        id[at] = (b * g.D + k) * 3 + c;
        return 0;
    });
}

// gather_indices: reads[(b D + k) 3 + c] counts the visits of an index, at[...] = the byte it loads
extern "C" int bt_walk_gather(int H, int W, int B, int sub, int32_t *reads, int64_t *at)
{
    const BlockGeom g = make_block_geom(H, W, B);
    return walk_tiles(g, sub, [&](int b, int k, int c) {
        const long long from = coef_pos(g, b, k, sub) * 3 + c;
        if (from < 0 || from >= g.k_stride) return -1;
        ++reads[(b * g.D + k) * 3 + c];
        at[(b * g.D + k) * 3 + c] = from;
        return 0;
    });
}

// crop_pixels: writes[at] counts the stores to byte at of the H x W x 3 frame, id[at] = (b D + j) 3 + c
// of the last one; *outside = the elements the crop drops
extern "C" int bt_walk_crop(int H, int W, int B, int32_t *writes, int32_t *id, int64_t *outside)
{
    const BlockGeom g = make_block_geom(H, W, B);
    *outside = 0;
    return walk_tiles(g, 0, [&](int b, int j, int c) {
        int y, x;
        pixel_yx(g, b, j, y, x);
        if (!in_frame(g, y, x)) {
            ++*outside;
            return 0;
        }
        const long long at = ((long long)y * g.W + x) * 3 + c;
        if (at < 0 || at >= g.rgb_stride) return -1;
        ++writes[at];
        id[at] = (b * g.D + j) * 3 + c;
        return 0;
    });
}
