// srh_speckle.hpp -- the per-element pieces of the speckle filter (srh_view_filter_speckles): which pixels
// are valid, which neighbours are joined, and the union-find over a plane of int32 labels.  Usable from host and gfx950
// device code: srh_speckle.hip runs them in LDS (one tile) and in device memory (across tile borders), and the CPU suite
// compiles this header with g++ and drives the very same routines sequentially (tests/test_speckle_host.py).
//
// The forest: L[i] is the parent of pixel i (its linear index y*w + x), L[i] == i a root, and L[i] <= i ALWAYS -- every
// link puts the larger index under the smaller -- so the forest has no cycle and a tree's root is its smallest member:
// the component's label.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRH_CHD __host__ __device__ __forceinline__
#else
#define SRH_CHD inline
#endif

// A label word that other lanes (other workgroups, on other XCDs with an L2 of their own) update while this lane reads it:
// on the device every access is a relaxed atomic at agent scope, which is served where the atomics are carried out and not
// from a cache line this CU or XCD may still hold; on the host (one thread) a plain load and a plain min.
#if defined(__HIP_DEVICE_COMPILE__)
#define SRH_CC_LOAD(p)     __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SRH_CC_MIN(p, v)   __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define SRH_CC_LOAD(p)     (*(p))
#define SRH_CC_MIN(p, v)   srh::cc::host_fetch_min((p), (v))
#endif

namespace srh {
namespace cc {

SRH_CHD int32_t host_fetch_min(int32_t *p, int32_t v) { const int32_t old = *p; if (v < old) *p = v; return old; }

// the default max_diff: `steps` depth steps of the run's parameters (srh_speckle_params.max_diff <= 0: steps = 2)
SRH_CHD double depth_steps(double min_depth, double max_depth, int num_depth_levels, double steps)
{
	return steps * ((max_depth - min_depth) / (double)(num_depth_levels - 1));
}

// a pixel takes part: mask WHITE, depth finite and > 0 (the -1 of "no peak", +-INF and NaN do not)
SRH_CHD bool valid(uint8_t mask, double d) { return mask == 1 && fabs(d) <= 1.7976931348623157e308 && d > 0; }
// two VALID 4-neighbours are joined (symmetric; in double)
SRH_CHD bool joined(double a, double b, double max_diff) { return fabs(a - b) <= max_diff; }

// The root of i's tree.  Every step goes to a strictly smaller index, so it ends.  A value another lane has replaced
// meanwhile is an older parent of the same pixel: still a member of its component, so the walk never leaves it.
SRH_CHD int32_t find(const int32_t *L, int32_t i)
{
	for (;;) {
		const int32_t p = SRH_CC_LOAD(L + i);
		if (p == i) return i;
		i = p;
	}
}

// Join the trees of a and b (monotone, lock-free).
// Termination: a pass either ends the loop or its fetch-min found `big` no longer a root and goes on with the value it
// got back, old < big, in big's place, so max(a, b) falls strictly from pass to pass (find only lowers a and b); it is an
// index >= 0, so at most max(a, b) + 1 passes happen, whatever other lanes do.  The loop holds no lock and never waits for
// another lane's progress.
// Correctness: labels only ever decrease (fetch-min) and L[i] <= i is kept.  A fetch-min that returns `big` linked the
// root big under small: joined.  One that returns old != big found big with the parent old < big: if old > small, big (and
// its subtree) now hangs under small and old's tree is still to be joined to small's; if old <= small nothing changed and
// big's tree is old's; either way joining old with small finishes the job, and that is the next pass.
SRH_CHD void unite(int32_t *L, int32_t a, int32_t b)
{
	for (;;) {
		a = find(L, a);
		b = find(L, b);
		if (a == b) return;
		const int32_t big = a > b ? a : b, small = a > b ? b : a;
		const int32_t old = SRH_CC_MIN(L + big, small);
		if (old == big) return;
		a = old;
		b = small;
	}
}

}  // namespace cc
}  // namespace srh
