// srh_fuse.hip -- depth-map fusion: the views' depth maps into one oriented point cloud (srh_mvs_fuse).
//
// Not in the reference (it writes one PLY per run and leaves merging to PMVS); the geometry is the reference's: a pixel's
// point is point_cloud_kernel's (unproject + pointFromDepth, the construction of both cross-checks) and the consistency
// test is MultiViewStereo::crossCheck's (multiviewstereo.cpp:666-729) without its early exit, the other view's point read
// from that view's point map instead of being unprojected again -- half the geometry, and one source for its bits.
//
// Per entry v of the slot list, in order on one stream:
//   fuse_view_kernel     one thread per pixel: members, support, the fused point, colour and normal into the view's staging
//                        planes; emit[pixel]; the block's number of emitted pixels; claims on entries u > v
//   fuse_scan_kernel     one workgroup: exclusive scan of the block counts on top of the points emitted so far
//   fuse_scatter_kernel  the emitted pixels to block offset + rank in the block (wave64 ballots): ascending (v, pixel)
// Determinism: the launch for v reads claimed[v] only and writes claimed[u], u > v, only, with plain byte stores of the
// value 1 (several threads may store the same 1); stream order separates the entries.  No atomic decides a position --
// the atomics below add up the info counters.
#include "srh_internal.hpp"
#include "srh_geom.hpp"
#include "srh_walk.hpp"

namespace srh {

__device__ __forceinline__ Vec3 cross3(Vec3 a, Vec3 b) {
	return v3(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);
}

// tangent along one image axis from the usable neighbours (lo: left / up, hi: right / down)
__device__ __forceinline__ bool fuse_tangent(bool lo_ok, Vec3 lo, bool hi_ok, Vec3 hi, Vec3 p, Vec3 &t) {
	if (lo_ok && hi_ok) { t = hi - lo; return true; }
	if (hi_ok) { t = hi - p; return true; }
	if (lo_ok) { t = p - lo; return true; }
	return false;
}

__global__ __launch_bounds__(SRH_FUSE_BLOCK)
void fuse_view_kernel(const ViewDev *__restrict__ views, const int32_t *__restrict__ slots, int nviews, int vi, srh_params P,
                      double thr, double gap, int min_views, const FuseViewDev *__restrict__ fv,
                      uint8_t *__restrict__ emit, FuseCloud stage, uint32_t *__restrict__ block_counts,
                      unsigned long long *__restrict__ counters)
{
	__shared__ unsigned wave_emitted[SRH_FUSE_BLOCK/64];
	const ViewDev &A = views[slots[vi]];
	const FuseViewDev me = fv[vi];
	const int W = A.w, H = A.h;
	const size_t npix = (size_t)W*H;
	const size_t i = (size_t)blockIdx.x*SRH_FUSE_BLOCK + threadIdx.x;
	unsigned n_point = 0, n_claimed = 0, n_unsup = 0, n_normal = 0;
	bool out = false;
	if (i < npix && me.valid[i] == 1) {
		if (me.claimed[i]) n_claimed = 1;
		else {
			const double s = P.image_scale;
			const Vec3 P1 = load3(me.pts + 3*i);
			// members in ascending list index; (v, i) itself at its own place
			Vec3 sum = v3(0, 0, 0);
			unsigned cr = 0, cg = 0, cb = 0;
			int m = 0;
			for (int u = 0; u < nviews; ++u) {
				Vec3 Pm;
				uint32_t colour;
				if (u == vi) { Pm = P1; colour = A.rgba[i]; }
				else {
					const ViewDev &B = views[slots[u]];
					Vec3 q = P1;
					if (!cam_project(B.cam, q)) continue;
					const double x2 = q.x*s, y2 = q.y*s;
					if (!(x2 >= 0 && y2 >= 0 && x2 < B.w && y2 < B.h)) continue;
					const size_t j = (size_t)((int)y2)*B.w + (int)x2;
					if (fv[u].valid[j] != 1) continue;
					Pm = load3(fv[u].pts + 3*j);
					const double nrm = norm(P1 - Pm);
					if (!(isfinite_d(nrm) && nrm < thr)) continue;
					colour = B.rgba[j];
				}
				sum = m ? sum + Pm : Pm;
				cr += colour & 255u; cg += (colour >> 8) & 255u; cb += (colour >> 16) & 255u;
				++m;
			}
			if (m < min_views) n_unsup = 1;
			else {
				out = true; n_point = 1;
				// the claims: the members of later entries, found again (a member list of up to 64 entries per thread would
				// live in scratch memory; the second projection of the few members is cheaper than that)
				for (int u = vi + 1; u < nviews; ++u) {
					const ViewDev &B = views[slots[u]];
					Vec3 q = P1;
					if (!cam_project(B.cam, q)) continue;
					const double x2 = q.x*s, y2 = q.y*s;
					if (!(x2 >= 0 && y2 >= 0 && x2 < B.w && y2 < B.h)) continue;
					const size_t j = (size_t)((int)y2)*B.w + (int)x2;
					if (fv[u].valid[j] != 1) continue;
					const double nrm = norm(P1 - load3(fv[u].pts + 3*j));
					if (isfinite_d(nrm) && nrm < thr) fv[u].claimed[j] = 1;
				}
				const double dm = (double)m;
				stage.xyz[3*i] = sum.x/dm; stage.xyz[3*i + 1] = sum.y/dm; stage.xyz[3*i + 2] = sum.z/dm;
				const unsigned um = (unsigned)m;
				stage.rgb[3*i] = (uint8_t)((2*cr + um)/(2*um));
				stage.rgb[3*i + 1] = (uint8_t)((2*cg + um)/(2*um));
				stage.rgb[3*i + 2] = (uint8_t)((2*cb + um)/(2*um));
				stage.nviews[i] = (uint8_t)m;
				// the normal, from this view's own point map
				const int x = (int)(i % W), y = (int)(i / W);
				const double depth = A.depth[i];
				const Vec3 zero = v3(0, 0, 0);
				auto usable = [&](bool inside, size_t k) {
					return inside && me.valid[k] == 1 && fabs(A.depth[k] - depth) <= gap;
				};
				const bool l_ok = usable(x > 0, i - 1), r_ok = usable(x + 1 < W, i + 1);
				const bool u_ok = usable(y > 0, i - W), d_ok = usable(y + 1 < H, i + W);
				Vec3 th, tv;
				const bool have_h = fuse_tangent(l_ok, l_ok ? load3(me.pts + 3*(i - 1)) : zero, r_ok, r_ok ? load3(me.pts + 3*(i + 1)) : zero, P1, th);
				const bool have_v = fuse_tangent(u_ok, u_ok ? load3(me.pts + 3*(i - W)) : zero, d_ok, d_ok ? load3(me.pts + 3*(i + W)) : zero, P1, tv);
				const Vec3 to_cam = load3(A.cam.C) - P1;
				Vec3 nv;
				bool has_normal = false;
				if (have_h && have_v) {
					nv = cross3(th, tv);
					const double len = norm(nv);
					if (isfinite_d(len) && len > 0) {
						nv = v3(nv.x/len, nv.y/len, nv.z/len);
						if (dot(nv, to_cam) < 0) nv = v3(-nv.x, -nv.y, -nv.z);
						has_normal = true;
					}
				}
				if (!has_normal) nv = normalized(to_cam);
				stage.nrm[3*i] = nv.x; stage.nrm[3*i + 1] = nv.y; stage.nrm[3*i + 2] = nv.z;
				stage.flags[i] = has_normal ? 1 : 0;
				n_normal = has_normal ? 1 : 0;
			}
		}
	}
	if (i < npix) emit[i] = out ? 1 : 0;
	// the block's count: one ballot per wave, added up by thread 0
	const unsigned long long b = __ballot(out);
	if ((threadIdx.x & 63) == 0) wave_emitted[threadIdx.x >> 6] = (unsigned)__popcll(b);
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned t = 0;
		for (int k = 0; k < SRH_FUSE_BLOCK/64; ++k) t += wave_emitted[k];
		block_counts[blockIdx.x] = t;
	}
	block_count_add(&counters[0], n_point);
	block_count_add(&counters[1], n_claimed);
	block_count_add(&counters[2], n_unsup);
	block_count_add(&counters[3], n_normal);
}

// One workgroup: thread t adds up a contiguous run of block counts, the runs' sums are scanned across the workgroup (shuffles
// inside a wave, LDS across the waves), then every thread writes its run's exclusive offsets on top of counters[4].
__global__ __launch_bounds__(SRH_FUSE_BLOCK)
void fuse_scan_kernel(const uint32_t *__restrict__ block_counts, int nblocks, unsigned long long *__restrict__ block_offs,
                      unsigned long long *__restrict__ counters)
{
	__shared__ unsigned long long wave_sum[SRH_FUSE_BLOCK/64];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int per = (nblocks + SRH_FUSE_BLOCK - 1)/SRH_FUSE_BLOCK;
	const int b0 = min(t*per, nblocks), b1 = min(b0 + per, nblocks);
	unsigned long long run = 0;
	for (int b = b0; b < b1; ++b) run += block_counts[b];
	unsigned long long incl = run;                                       // inclusive scan over the wave's 64 runs
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long up = __shfl_up(incl, d, 64);
		if (lane >= d) incl += up;
	}
	if (lane == 63) wave_sum[wave] = incl;
	__syncthreads();
	unsigned long long base = counters[4], all = 0;
	for (int k = 0; k < SRH_FUSE_BLOCK/64; ++k) { if (k < wave) base += wave_sum[k]; all += wave_sum[k]; }
	unsigned long long off = base + (incl - run);
	for (int b = b0; b < b1; ++b) { block_offs[b] = off; off += block_counts[b]; }
	__syncthreads();                                                     // (every thread has read counters[4])
	if (t == 0) counters[4] += all;
}

__global__ __launch_bounds__(SRH_FUSE_BLOCK)
void fuse_scatter_kernel(int vi, size_t npix, const uint8_t *__restrict__ emit, FuseCloud stage,
                         const unsigned long long *__restrict__ block_offs, FuseCloud out, unsigned long long cap)
{
	__shared__ unsigned wave_emitted[SRH_FUSE_BLOCK/64];
	const size_t i = (size_t)blockIdx.x*SRH_FUSE_BLOCK + threadIdx.x;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool e = i < npix && emit[i] == 1;
	const unsigned long long b = __ballot(e);
	if (lane == 0) wave_emitted[wave] = (unsigned)__popcll(b);
	__syncthreads();
	if (!e) return;
	unsigned long long pos = block_offs[blockIdx.x] + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
	for (int k = 0; k < wave; ++k) pos += wave_emitted[k];
	if (pos >= cap) return;                                              // (cannot happen: cap = pixels with a point)
	out.xyz[3*pos] = stage.xyz[3*i]; out.xyz[3*pos + 1] = stage.xyz[3*i + 1]; out.xyz[3*pos + 2] = stage.xyz[3*i + 2];
	out.nrm[3*pos] = stage.nrm[3*i]; out.nrm[3*pos + 1] = stage.nrm[3*i + 1]; out.nrm[3*pos + 2] = stage.nrm[3*i + 2];
	out.rgb[3*pos] = stage.rgb[3*i]; out.rgb[3*pos + 1] = stage.rgb[3*i + 1]; out.rgb[3*pos + 2] = stage.rgb[3*i + 2];
	out.nviews[pos] = stage.nviews[i];
	out.flags[pos] = stage.flags[i];
	out.src[2*pos] = vi; out.src[2*pos + 1] = (int32_t)i;
}

static unsigned fuse_blocks(size_t npix) { return (unsigned)((npix + SRH_FUSE_BLOCK - 1)/SRH_FUSE_BLOCK); }

void launch_fuse_view(hipStream_t st, const ViewDev *views, const int32_t *slots_dev, int nviews, int vi, int w, int h,
                      const srh_params &P, double thr, double gap, int min_views, const FuseViewDev *fv,
                      uint8_t *emit, FuseCloud stage, uint32_t *block_counts, unsigned long long *counters)
{
	hipLaunchKernelGGL(fuse_view_kernel, dim3(fuse_blocks((size_t)w*h)), dim3(SRH_FUSE_BLOCK), 0, st,
	                   views, slots_dev, nviews, vi, P, thr, gap, min_views, fv, emit, stage, block_counts, counters);
}

void launch_fuse_scan(hipStream_t st, const uint32_t *block_counts, int nblocks, unsigned long long *block_offs,
                      unsigned long long *counters)
{
	hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(SRH_FUSE_BLOCK), 0, st, block_counts, nblocks, block_offs, counters);
}

void launch_fuse_scatter(hipStream_t st, int vi, size_t npix, const uint8_t *emit, FuseCloud stage,
                         const unsigned long long *block_offs, FuseCloud out, unsigned long long cap)
{
	hipLaunchKernelGGL(fuse_scatter_kernel, dim3(fuse_blocks(npix)), dim3(SRH_FUSE_BLOCK), 0, st,
	                   vi, npix, emit, stage, block_offs, out, cap);
}

} // namespace srh
