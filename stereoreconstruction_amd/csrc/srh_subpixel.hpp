// srh_subpixel.hpp -- launch wrappers of srh_subpixel.hip (option "subpixel"); all asynchronous on `st`.
#pragma once

#include "srh_internal.hpp"

namespace srh {

// rows [y0, y0 + nrows) of the reference view: every pixel's n- and n+ into neigh[pixel][4] ((-1, -1) = none) and its
// provisional class into cls -- NONE, NO_NEIGHBOUR, or REFINED for a pixel the refine kernel still has to decide.
// win_xy: the kept winners; tdist: label_plane_dist per label (label_plane_table_kernel), or null
void launch_subpixel_neighbours(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P,
                                int y0, int nrows, const double *tdist, const int32_t *win_xy, int32_t *neigh, uint8_t *cls);
// the same rows: the costs of n- and n+ in the reference's arithmetic from the band's window buffer (either layout, as
// launch_twoview_winner_costs), c0 from min_cost; delta and the final class of every pixel, the depth of the refined ones
void launch_subpixel_refine(hipStream_t st, const ViewDev *views, int ref, int oth, int width, const srh_params &P, int kind,
                            int y0, int nrows, const double *wbuf, bool wimg, const int32_t *win_xy, const double *min_cost,
                            const int32_t *neigh, uint8_t *cls, double *delta);

} // namespace srh
