// srh_mvs_subpixel.hpp -- launch wrappers of srh_mvs_subpixel.hip (srh_mvs_view_subpixel); all asynchronous
// on `st`.
#pragma once

#include "srh_internal.hpp"

namespace srh {

// Chebyshev radius of the narrowed winner search around the pixel of the neighbour view that holds the projection of the
// reference pixel's point at its depth (DESIGN.md 4o derives why 2 suffices; 3 leaves a pixel of room)
#define SRH_MVSSUB_RADIUS 3

// counters of one call (device memory, zeroed by the caller): [0..5] pixels per SRH_SUBPX_* class, [6] refined pixels with
// delta != 0, [7] pixels the narrowed search handed to the exhaustive one
#define SRH_MVSSUB_COUNTERS 8

// rows [y0, y0 + nrows) of view `ref`: every pixel's winner (index into the neighbour list, cx, cy; (-1, -1, -1) = none)
// into win[pixel][3], its n- and n+ into neigh[pixel][4] ((-1, -1) = none) and its provisional class into cls -- NONE,
// NO_WINNER, NO_NEIGHBOUR, or REFINED for a pixel the refine kernel still has to decide.  exhaustive: every curve pixel of
// every neighbour is triangulated; else only those within SRH_MVSSUB_RADIUS of the projected point, and a pixel without a
// winner there is searched exhaustively (counted in cnt[7])
void launch_mvs_subpixel_search(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh_slots, int nneigh, int width,
                                const srh_params &P, int y0, int nrows, bool exhaustive, int32_t *win, int32_t *neigh,
                                uint8_t *cls, unsigned long long *cnt);
// the same rows, from the band's window buffer (tile-major, as launch_weights fills it for row y0 = band row 0): c-, c0, c+
// in the arithmetic of mvs_cost, delta and the final class of every pixel, the depth of the refined ones; cnt[0..6]
void launch_mvs_subpixel_refine(hipStream_t st, const ViewDev *views, int ref, const int32_t *neigh_slots, int nneigh, int width,
                                const srh_params &P, int y0, int nrows, const double *wbuf, const int32_t *win,
                                const int32_t *neigh, uint8_t *cls, double *delta, unsigned long long *cnt);

} // namespace srh
