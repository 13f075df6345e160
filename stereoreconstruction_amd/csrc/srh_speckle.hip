// srh_speckle.hip -- speckle filter of one view's depth map: 4-connected components of the valid pixels whose depths differ
// by at most max_diff, and the components smaller than min_size overwritten (srh_view_filter_speckles).
// The validity and join predicates and the union-find are srh_speckle.hpp's.  Two int32 planes A and B:
//   speckle_tile_kernel     one workgroup per 32x32 tile: the tile's joins in an LDS union-find, then
//                           A[pixel] = global index of the tile-local root (-1: not valid)
//   speckle_merge_kernel    one lane per pixel pair across a tile border: cc::unite in device memory, every access of A a
//                           relaxed agent-scope atomic
//   speckle_flatten_kernel  B[pixel] = root of the pixel in A (A is no longer written: plain loads)
//   speckle_count_kernel    size[root] in A (zeroed): a wave combines its lanes that share a root before it adds
//   speckle_apply_kernel    the reject value where size[B[pixel]] < min_size, and the five counters of srh_speckle_info
#include "srh_internal.hpp"
#include "srh_speckle.hpp"

namespace srh {

#define SPK_T 32                     // tile side
#define SPK_THREADS 256
#define SPK_CHUNKS 8                 // 64-pixel chunks a wave of the count kernel walks

__global__ __launch_bounds__(SPK_THREADS) void speckle_tile_kernel(const uint8_t *__restrict__ mask, const double *__restrict__ D,
                                                                   int w, int h, double max_diff, int32_t *__restrict__ A)
{
	__shared__ double val[SPK_T*SPK_T];          // the pixel's depth, NaN where it is not valid (or outside the image)
	__shared__ int32_t lab[SPK_T*SPK_T];
	const int x0 = blockIdx.x*SPK_T, y0 = blockIdx.y*SPK_T;
	for (int k = threadIdx.x; k < SPK_T*SPK_T; k += SPK_THREADS) {
		const int x = x0 + k % SPK_T, y = y0 + k / SPK_T;
		double d = __builtin_nan("");
		if (x < w && y < h) {
			const size_t g = (size_t)y*w + x;
			const double v = D[g];
			if (cc::valid(mask[g], v)) d = v;
		}
		val[k] = d;
		lab[k] = k;
	}
	__syncthreads();
	for (int k = threadIdx.x; k < SPK_T*SPK_T; k += SPK_THREADS) {
		const double d = val[k];
		if (d != d) continue;
		if (k % SPK_T + 1 < SPK_T) { const double e = val[k + 1];     if (e == e && cc::joined(d, e, max_diff)) cc::unite(lab, k, k + 1); }
		if (k / SPK_T + 1 < SPK_T) { const double e = val[k + SPK_T]; if (e == e && cc::joined(d, e, max_diff)) cc::unite(lab, k, k + SPK_T); }
	}
	__syncthreads();
	for (int k = threadIdx.x; k < SPK_T*SPK_T; k += SPK_THREADS) {
		const int x = x0 + k % SPK_T, y = y0 + k / SPK_T;
		if (x >= w || y >= h) continue;
		int32_t out = -1;
		if (val[k] == val[k]) {
			const int32_t r = cc::find(lab, k);
			out = (int32_t)((size_t)(y0 + r / SPK_T)*w + (x0 + r % SPK_T));
		}
		A[(size_t)y*w + x] = out;
	}
}

// pairs [0, nv): across the vertical borders (x = bx*SPK_T - 1 | bx*SPK_T), then across the horizontal ones
__global__ __launch_bounds__(SPK_THREADS) void speckle_merge_kernel(const double *__restrict__ D, int w, int h, double max_diff,
                                                                    int32_t *A)
{
	const int nbx = (w - 1) / SPK_T, nby = (h - 1) / SPK_T;      // borders inside the image
	const long long nv = (long long)nbx*h, total = nv + (long long)nby*w;
	const long long q = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	if (q >= total) return;
	size_t a, b;
	if (q < nv) {
		const int y = (int)(q / nbx), bx = (int)(q % nbx) + 1;
		a = (size_t)y*w + (size_t)bx*SPK_T - 1;
		b = a + 1;
	} else {
		const long long j = q - nv;
		const int by = (int)(j / w) + 1, x = (int)(j % w);
		a = ((size_t)by*SPK_T - 1)*w + x;
		b = a + w;
	}
	// (-1 = not valid: written by the tile kernel, before this launch, and never changed)
	if (SRH_CC_LOAD(A + a) < 0 || SRH_CC_LOAD(A + b) < 0) return;
	if (cc::joined(D[a], D[b], max_diff)) cc::unite(A, (int32_t)a, (int32_t)b);
}

__global__ __launch_bounds__(SPK_THREADS) void speckle_flatten_kernel(const int32_t *__restrict__ A, size_t n, int32_t *__restrict__ B)
{
	const size_t i = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	int32_t r = A[i];
	if (r >= 0)
		for (int32_t p; (p = A[r]) != r;) r = p;
	B[i] = r;
}

// size[root] += members.  A wave walks SPK_CHUNKS chunks of 64 consecutive pixels.  Per chunk, up to 4 times: the lanes
// that share the root of the first lane still to be counted are counted by one ballot; the wave keeps ONE (root, count)
// pending and adds it to memory only when another root takes its place -- a surface that fills the wave's pixels costs one
// atomic per wave, not one per pixel.  What 4 rounds leave adds per lane.  Integer adds: the sums do not depend on the order.
__global__ __launch_bounds__(SPK_THREADS) void speckle_count_kernel(const int32_t *__restrict__ B, size_t n, int32_t *__restrict__ size)
{
	const unsigned lane = threadIdx.x & 63;
	const size_t wave = (size_t)blockIdx.x*(SPK_THREADS/64) + (threadIdx.x >> 6);
	int32_t pend_root = -1, pend_cnt = 0;                      // wave-uniform
	for (int c = 0; c < SPK_CHUNKS; ++c) {
		const size_t i = (wave*SPK_CHUNKS + c)*64 + lane;
		const int32_t r = i < n ? B[i] : -1;
		bool todo = r >= 0;
		for (int round = 0; round < 4; ++round) {
			const unsigned long long act = __ballot(todo);
			if (!act) break;
			const int32_t lead = __shfl(r, __ffsll((long long)act) - 1);
			const bool same = todo && r == lead;
			const int32_t cnt = (int32_t)__popcll(__ballot(same));
			if (lead == pend_root) pend_cnt += cnt;
			else {
				if (pend_cnt && lane == 0) atomicAdd(size + pend_root, pend_cnt);
				pend_root = lead;
				pend_cnt = cnt;
			}
			todo = todo && !same;
		}
		if (todo) atomicAdd(size + r, 1);
	}
	if (pend_cnt && lane == 0) atomicAdd(size + pend_root, pend_cnt);
}

// counters: [0] valid, [1] components, [2] removed components, [3] removed pixels, [4] largest component.
// All five live in one cache line: a ballot and an atomic per wave and counter (the filter kernels' wave_count) made this
// kernel 1.8 ms of the stage's 1.9 on a 1920x1080 map, all of it waiting for that line.  So a fixed grid strides over the
// pixels, every lane counts in registers, and a workgroup adds its sums once: at most 5 atomics per workgroup.
#define SPK_APPLY_BLOCKS 1024
__global__ __launch_bounds__(SPK_THREADS) void speckle_apply_kernel(const int32_t *__restrict__ B, const int32_t *__restrict__ size,
                                                                    size_t n, int32_t min_size, double reject,
                                                                    double *__restrict__ D, unsigned long long *__restrict__ cnt)
{
	__shared__ int32_t part[SPK_THREADS/64][5];
	int32_t c[5] = { 0, 0, 0, 0, 0 };                    // (a lane sees at most 2^31 / (1024*256) pixels)
	for (size_t i = (size_t)blockIdx.x*SPK_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x*SPK_THREADS) {
		const int32_t r = B[i];
		if (r < 0) continue;
		const int32_t sz = size[r];
		const bool root = (size_t)r == i, removed = sz < min_size;
		if (removed) D[i] = reject;
		c[0] += 1;
		c[1] += root;
		c[2] += root && removed;
		c[3] += removed;
		if (root) c[4] = max(c[4], sz);
	}
	for (int s = 32; s > 0; s >>= 1) {
		for (int k = 0; k < 4; ++k) c[k] += __shfl_xor(c[k], s);
		c[4] = max(c[4], __shfl_xor(c[4], s));
	}
	if ((threadIdx.x & 63) == 0)
		for (int k = 0; k < 5; ++k) part[threadIdx.x >> 6][k] = c[k];
	__syncthreads();
	if (threadIdx.x < 5) {
		const int k = threadIdx.x;
		int32_t v = part[0][k];
		for (int wv = 1; wv < SPK_THREADS/64; ++wv) v = k < 4 ? v + part[wv][k] : max(v, part[wv][k]);
		if (v > 0) { if (k < 4) atomicAdd(cnt + k, (unsigned long long)v); else atomicMax(cnt + 4, (unsigned long long)v); }
	}
}

void launch_speckle_tiles(hipStream_t st, const uint8_t *mask, const double *D, int w, int h, double max_diff, int32_t *A)
{
	hipLaunchKernelGGL(speckle_tile_kernel, dim3((unsigned)((w + SPK_T - 1)/SPK_T), (unsigned)((h + SPK_T - 1)/SPK_T)), dim3(SPK_THREADS),
	                   0, st, mask, D, w, h, max_diff, A);
}

void launch_speckle_merge(hipStream_t st, const double *D, int w, int h, double max_diff, int32_t *A)
{
	const long long total = (long long)((w - 1)/SPK_T)*h + (long long)((h - 1)/SPK_T)*w;
	if (total <= 0) return;
	hipLaunchKernelGGL(speckle_merge_kernel, dim3((unsigned)((total + SPK_THREADS - 1)/SPK_THREADS)), dim3(SPK_THREADS), 0, st,
	                   D, w, h, max_diff, A);
}

void launch_speckle_flatten(hipStream_t st, const int32_t *A, size_t n, int32_t *B)
{
	hipLaunchKernelGGL(speckle_flatten_kernel, dim3((unsigned)((n + SPK_THREADS - 1)/SPK_THREADS)), dim3(SPK_THREADS), 0, st, A, n, B);
}

void launch_speckle_count(hipStream_t st, const int32_t *B, size_t n, int32_t *size)
{
	const size_t per_block = (size_t)SPK_THREADS*SPK_CHUNKS;
	hipLaunchKernelGGL(speckle_count_kernel, dim3((unsigned)((n + per_block - 1)/per_block)), dim3(SPK_THREADS), 0, st, B, n, size);
}

void launch_speckle_apply(hipStream_t st, const int32_t *B, const int32_t *size, size_t n, int min_size, double reject, double *D,
                          unsigned long long *cnt)
{
	const size_t blocks = (n + SPK_THREADS - 1)/SPK_THREADS;
	hipLaunchKernelGGL(speckle_apply_kernel, dim3((unsigned)(blocks < SPK_APPLY_BLOCKS ? blocks : SPK_APPLY_BLOCKS)), dim3(SPK_THREADS), 0, st,
	                   B, size, n, (int32_t)min_size, reject, D, cnt);
}

}  // namespace srh
