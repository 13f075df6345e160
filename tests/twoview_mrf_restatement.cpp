// CPU restatement of TwoViewStereo's MRF stage (include/stereo_recon_hip.h, "TwoViewStereo, MRF stage"):
// depthFromLabel, the fill rule, and the optimiser -- sequential TRW-S exactly as oracle/sr_oracle.c (sro_mvs_mrf) writes
// it down, with L = D labels and trws_V replaced by lambda * min((double)|ks - kd|, smooth_max).  PARITY UNPINNED: the
// reference's branch is compile-time dead and its solver is not in its tree.
//
// The message update exists in two forms: the direct O(L^2) one (form 0), and the windowed one the kernel uses (form 1):
//     M[kd] = min( min_{|d| < smooth_max} (buf[kd + d] + lambda*|d|),  min_ks buf[ks] + lambda*smooth_max )
// tests/test_twoview_mrf_restatement.py holds them against each other bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Trws {
	int w, h, L, form;
	double lambda, smax;
	const double *D;             // n*L
	std::vector<double> M;       // n*2*L, [pixel][0: edge to x+1, 1: edge to y+1][label]
	std::vector<int32_t> ans;
	std::vector<double> buf, Di;
};

double V(const Trws &t, int ks, int kd) {
	const double d = (double)std::abs(ks - kd);
	return t.lambda*(d < t.smax ? d : t.smax);                        // one product
}

// new message over an edge, written over the stored (reverse) message; returns the constant taken out
double update(Trws &t, double *M, const double *Di) {
	const int L = t.L;
	double *buf = t.buf.data(), delta = 0;
	for (int ks = 0; ks < L; ks++) buf[ks] = 0.5*Di[ks] - M[ks];
	if (t.form == 0) {
		for (int kd = 0; kd < L; kd++) {
			double vmin = buf[0] + V(t, 0, kd);
			for (int ks = 1; ks < L; ks++) {
				const double v = buf[ks] + V(t, ks, kd);
				if (vmin > v) vmin = v;
			}
			M[kd] = vmin;
		}
	} else {
		double g = buf[0];
		for (int ks = 1; ks < L; ks++) if (g > buf[ks]) g = buf[ks];
		const double gm = g + t.lambda*t.smax;
		for (int kd = 0; kd < L; kd++) {
			double m = buf[kd] + t.lambda*0.0;
			for (int d = 1; (double)d < t.smax; d++) {
				const double c = t.lambda*(double)d;
				if (kd - d >= 0) { const double v = buf[kd - d] + c; if (m > v) m = v; }
				if (kd + d < L)  { const double v = buf[kd + d] + c; if (m > v) m = v; }
			}
			if (m > gm) m = gm;
			M[kd] = m;
		}
	}
	for (int kd = 0; kd < L; kd++) if (kd == 0 || delta > M[kd]) delta = M[kd];
	for (int kd = 0; kd < L; kd++) M[kd] -= delta;
	return delta;
}

void gather(Trws &t, int x, int y, double *Di) {
	const int L = t.L, w = t.w, h = t.h;
	const size_t n = (size_t)y*w + x;
	const double *M = t.M.data() + n*2*L;
	for (int k = 0; k < L; k++) Di[k] = t.D[n*L + k];
	if (x > 0)     for (int k = 0; k < L; k++) Di[k] += (M - 2*L)[k];                 // (x-1,y) -> (x,y)
	if (y > 0)     for (int k = 0; k < L; k++) Di[k] += (M - (size_t)2*w*L + L)[k];   // (x,y-1) -> (x,y)
	if (x < w - 1) for (int k = 0; k < L; k++) Di[k] += M[k];                         // (x+1,y) -> (x,y)
	if (y < h - 1) for (int k = 0; k < L; k++) Di[k] += (M + L)[k];                   // (x,y+1) -> (x,y)
}

double sweep(Trws &t) {
	const int L = t.L, w = t.w, h = t.h;
	double *Di = t.Di.data(), lower = 0;
	for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {                         // forward
		double *M = t.M.data() + ((size_t)y*w + x)*2*L;
		gather(t, x, y, Di);
		if (x < w - 1) update(t, M, Di);
		if (y < h - 1) update(t, M + L, Di);
	}
	for (int y = h - 1; y >= 0; y--) for (int x = w - 1; x >= 0; x--) {               // backward
		double *M = t.M.data() + ((size_t)y*w + x)*2*L;
		gather(t, x, y, Di);
		double vmin = Di[0];
		for (int k = 1; k < L; k++) if (vmin > Di[k]) vmin = Di[k];
		for (int k = 0; k < L; k++) Di[k] -= vmin;
		lower += vmin;
		if (x > 0) lower += update(t, M - 2*L, Di);
		if (y > 0) lower += update(t, M - (size_t)2*w*L + L, Di);
	}
	for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {                         // read the labels off
		const size_t n = (size_t)y*w + x;
		const double *M = t.M.data() + n*2*L;
		for (int k = 0; k < L; k++) Di[k] = t.D[n*L + k];
		if (x > 0)     for (int k = 0; k < L; k++) Di[k] += V(t, t.ans[n - 1], k);
		if (y > 0)     for (int k = 0; k < L; k++) Di[k] += V(t, t.ans[n - w], k);
		if (x < w - 1) for (int k = 0; k < L; k++) Di[k] += M[k];
		if (y < h - 1) for (int k = 0; k < L; k++) Di[k] += (M + L)[k];
		double best = Di[0];
		int a = 0;
		for (int k = 1; k < L; k++) if (best > Di[k]) { best = Di[k]; a = k; }         // the lowest index wins a tie
		t.ans[n] = a;
	}
	return lower;
}

double energy_of(const Trws &t, const int32_t *ans) {
	const int L = t.L, w = t.w, h = t.h;
	double data = 0, smooth = 0;
	for (size_t n = 0; n < (size_t)w*h; n++) data += t.D[n*L + ans[n]];
	for (int y = 0; y < h; y++) for (int x = 1; x < w; x++) { const size_t n = (size_t)y*w + x; smooth += V(t, ans[n], ans[n - 1]); }
	for (int y = 1; y < h; y++) for (int x = 0; x < w; x++) { const size_t n = (size_t)y*w + x; smooth += V(t, ans[n], ans[n - w]); }
	return data + smooth;
}

} // namespace

extern "C" {

// depthFromLabel (twoviewstereo.cpp:981-985, non-uniform)
double tvm_depth_from_label(int label, int num_depth_levels, double min_depth, double max_depth) {
	double t = label / (num_depth_levels - 1.0);
	t /= (5 - 4*t);
	return min_depth*(1 - t) + max_depth*t;
}

// WINDOW_SIZE*BAD_RET (:258): what std::fill leaves where a label is never costed
double tvm_fill_value(int window_radius, double bad_ret) { return (2*window_radius + 1)*bad_ret; }

// the energy of a labelling (E = sum D_p(l_p) + sum_(p,q) lambda*min(|l_p - l_q|, smooth_max), 4-connected grid)
double tvm_energy(int w, int h, int L, const double *costs, double lambda, double smooth_max, const int32_t *labels) {
	Trws t;
	t.w = w; t.h = h; t.L = L; t.form = 0; t.lambda = lambda; t.smax = smooth_max; t.D = costs;
	return energy_of(t, labels);
}

// The optimiser on data costs [pixel][L].  form 0: direct messages, 1: windowed.  mask (may be null): 1 <=> WHITE.
// Outputs (each may be null): depth (w*h: depthFromLabel(label) where the mask is WHITE, NaN elsewhere), labels (w*h),
// messages (w*h*2*L), info = {iterations, energy_initial, energy_final, lower_bound}.
void tvm_optimize(int w, int h, int L, const double *costs, const uint8_t *mask, double lambda, double smooth_max,
                  int max_iters, double min_energy_drop, int form, double min_depth, double max_depth,
                  double *depth, int32_t *labels, double *messages, double *info) {
	Trws t;
	const size_t n = (size_t)w*h;
	t.w = w; t.h = h; t.L = L; t.form = form; t.lambda = lambda; t.smax = smooth_max; t.D = costs;
	t.M.assign(n*2*L, 0.0);                                            // messages zero
	t.ans.assign(n, 0);                                                // labelling all 0
	t.buf.resize(L); t.Di.resize(L);
	// twoviewstereo.cpp:378-390
	double energy = energy_of(t, t.ans.data()), prev = 0.0, lower = 0.0;
	const double e0 = energy;
	int num_iters = max_iters, iters = 0;
	do {
		prev = energy;
		lower = sweep(t);
		energy = energy_of(t, t.ans.data());
		++iters;
	} while (prev - energy > min_energy_drop && num_iters-- > 0);
	if (depth)
		for (size_t p = 0; p < n; p++)
			depth[p] = (!mask || mask[p] == 1) ? tvm_depth_from_label(t.ans[p], L, min_depth, max_depth) : __builtin_nan("");
	if (labels) memcpy(labels, t.ans.data(), n*sizeof(int32_t));
	if (messages) memcpy(messages, t.M.data(), n*2*L*sizeof(double));
	if (info) { info[0] = iters; info[1] = e0; info[2] = energy; info[3] = lower; }
}

}
