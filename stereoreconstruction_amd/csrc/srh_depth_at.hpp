// srh_depth_at.hpp -- what the two sub-pixel stages share (srh_subpixel.hip: option "subpixel", DESIGN.md 4n;
// srh_mvs_subpixel.hip: srh_mvs_view_subpixel): the triangulation at a real-valued position of the other
// view and the curve visitor that keeps the winner's visited neighbours.
#pragma once

#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"

namespace srh {

// candidate_depth (srh_walk.hpp) at a position of the other view given in scaled pixel coordinates (a pixel's centre is
// cx + 0.5: the same operations as candidate_depth for an integer candidate)
__device__ __forceinline__ double candidate_depth_at(const srh_camera &refcam, const srh_camera &othcam, const srh_params &P,
                                                     const Ray &ray, double qx, double qy)
{
	const Ray ray2 = cam_unproject(othcam, qx / P.image_scale, qy / P.image_scale);
	Vec3 p1, p2;
	closest_points(ray, ray2, p1, p2);
	p1 = p1 + p2;
	p1 = p1*0.5;
	return cam_local_z(refcam, p1);
}

// bit (dy + 1)*3 + (dx + 1) of `mask` for every visited pixel at Chebyshev distance 1 from (wx, wy): ascending bits are
// ascending (qy, qx)
struct AdjacencyVisitor {
	int wx, wy;
	unsigned mask;
	__device__ __forceinline__ void operator()(int cx, int cy) {
		const int dx = cx - wx, dy = cy - wy;
		if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && (dx | dy) != 0) mask |= 1u << ((dy + 1)*3 + (dx + 1));
	}
};

} // namespace srh
