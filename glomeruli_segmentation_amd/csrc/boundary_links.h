// The test that the analyses which search along instance boundaries (boundary_dist.hip, zones.hip, lesions.hip) share: "is this
// pixel a boundary pixel of a valid instance".  Their exactness arguments rest on one definition of a boundary, so it is written
// once, here; the links of a row to such pixels end in kLinkNone (slide_map_plan.h).  A device header under the rules of
// wave_block.h; it holds no loop.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

// Is (x, y), a pixel of the map, a boundary pixel of a valid instance of L?  id: its label (any value where the answer is no).
// A valid instance is a label in 1..n; a boundary pixel has a 4-neighbour that carries another value or lies outside the map.
// No branch: the five loads go out together.  A neighbour beyond the map's edge is read at the pixel itself, and the edge
// test beside it decides.
__device__ inline bool boundary_pixel(const int *__restrict__ L, int n, int H, int W, int y, int x, int &id)
{
    const size_t i = (size_t)y * W + x;
    const int a = L[i];
    const int l = L[i - (x > 0 ? 1 : 0)], r = L[i + (x < W - 1 ? 1 : 0)];
    const int u = L[i - (y > 0 ? (size_t)W : 0)], d = L[i + (y < H - 1 ? (size_t)W : 0)];
    id = a;
    return (a >= 1) & (a <= n) & ((x == 0) | (l != a) | (x == W - 1) | (r != a) | (y == 0) | (u != a) | (y == H - 1) | (d != a));
}

}  // namespace gs
