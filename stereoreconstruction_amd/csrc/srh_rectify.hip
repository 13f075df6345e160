// srh_rectify.hip -- the warp of a view onto a rectified camera and the way back for its depth map (srh_twoview_rectify,
// srh_view_rectify_map, srh_view_depth_unrectify).  The per-pixel arithmetic is srh_rectify.hpp's.
//   rectify_warp_kernel    one lane per destination pixel: the map (u, v), the bilinear bytes, the mask
//   unrectify_kernel       one lane per pixel of the original view: the rectified pixel its ray falls into, its depth
// Workgroups of 64 x 4: a wave is 64 consecutive columns of one row, so neighbouring lanes read neighbouring texels (the
// gather is served by L2) and write consecutive words.  About 150 FP64 operations and 16 gathered bytes per pixel: no LDS.
#include "srh_internal.hpp"
#include "srh_rectify.hpp"

namespace srh {

#define RCT_BX 64
#define RCT_BY 4

// uv (optional): out_w*out_h pairs; rgba / mask (optional, both or neither): the warped view
__global__ __launch_bounds__(RCT_BX*RCT_BY) void rectify_warp_kernel(const ViewDev *__restrict__ views, int src, srh_camera rect_cam,
                                                                       int out_w, int out_h, double s, double *__restrict__ uv,
                                                                       uint32_t *__restrict__ rgba, uint8_t *__restrict__ mask)
{
	const int x = (int)(blockIdx.x*RCT_BX + threadIdx.x), y = (int)(blockIdx.y*RCT_BY + threadIdx.y);
	if (x >= out_w || y >= out_h) return;
	const ViewDev &S = views[src];
	const size_t i = (size_t)y*out_w + x;
	double u, v;
	const bool ok = rect::warp_map(rect_cam, S.cam, x, y, s, u, v);
	if (uv) { uv[2*i] = u; uv[2*i + 1] = v; }
	if (!rgba) return;
	uint32_t px = 0;
	uint8_t m = 0;
	if (ok) rect::warp_pixel(S.rgba, S.mask, S.w, S.h, u, v, px, m);
	rgba[i] = px;
	mask[i] = m;
}

__global__ __launch_bounds__(RCT_BX*RCT_BY) void unrectify_kernel(const ViewDev *__restrict__ views, int rect_slot, int dst_slot, double s,
                                                                    int32_t *__restrict__ index)
{
	const ViewDev &D = views[dst_slot];
	const ViewDev &R = views[rect_slot];
	const int x = (int)(blockIdx.x*RCT_BX + threadIdx.x), y = (int)(blockIdx.y*RCT_BY + threadIdx.y);
	if (x >= D.w || y >= D.h) return;
	const size_t i = (size_t)y*D.w + x;
	double depth = __builtin_nan("");
	int64_t j = -1;
	if (D.mask[i] == 1) {
		Ray ray;
		j = rect::unrectify_index(D.cam, R.cam, x, y, s, R.w, R.h, ray);
		if (j >= 0) depth = rect::unrectify_depth(D.cam, R.cam, ray, R.depth[j]);
	}
	D.depth[i] = depth;
	if (index) index[i] = (int32_t)j;
}

static dim3 rct_grid(int w, int h) { return dim3((unsigned)((w + RCT_BX - 1)/RCT_BX), (unsigned)((h + RCT_BY - 1)/RCT_BY)); }

void launch_rectify_warp(hipStream_t st, const ViewDev *views, int src, const srh_camera &rect_cam, int out_w, int out_h, double s,
                         double *uv, uint32_t *rgba, uint8_t *mask)
{
	hipLaunchKernelGGL(rectify_warp_kernel, rct_grid(out_w, out_h), dim3(RCT_BX, RCT_BY), 0, st, views, src, rect_cam, out_w, out_h, s,
	                   uv, rgba, mask);
}

void launch_unrectify(hipStream_t st, const ViewDev *views, int rect_slot, int dst_slot, int w, int h, double s, int32_t *index)
{
	hipLaunchKernelGGL(unrectify_kernel, rct_grid(w, h), dim3(RCT_BX, RCT_BY), 0, st, views, rect_slot, dst_slot, s, index);
}

}  // namespace srh
