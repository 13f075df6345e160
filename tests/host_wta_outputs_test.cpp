// host_wta_outputs_test.cpp -- the Qt-free TwoViewStereo (stereoreconstruction_amd/host) keeping the by-products of its
// WTA scan (setKeepWtaOutputs):
//   host_wta_outputs_test in.bin out.bin flags [mrf]
// in.bin: the format of host_api_test.cpp (two views, with masks).  out.bin: the left and the right depth map (w*h doubles
// each), eight int32 element counts, then the eight vectors in the order leftWinners, leftRunnersUp, leftMinCosts,
// leftSecondCosts, rightWinners, rightRunnersUp, rightMinCosts, rightSecondCosts.  tests/test_gpu_wta_outputs.py checks
// them against the C-ABI download; tests/test_wta_outputs_host.py compiles and links it without a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
template <class T> static void wr(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
	if (argc < 4) { fprintf(stderr, "usage: %s in.bin out.bin flags [mrf]\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	int32_t hdr[6];
	double dh[4];
	rd(f, hdr, 6); rd(f, dh, 4);
	const int nv = hdr[0], w = hdr[1], h = hdr[2];
	if (nv != 2) { fprintf(stderr, "two views expected\n"); return 2; }
	std::vector<CameraPtr> cams;
	std::vector<Image> imgs, masks;
	for (int v = 0; v < 2; ++v) {
		double K[9], R[9], t[3]; LensDistortions dist;
		rd(f, K, 9); rd(f, R, 9); rd(f, t, 3); rd(f, dist.data(), 5);
		CameraPtr cam(new Camera(std::to_string(v), "cam" + std::to_string(v)));
		cam->set(K, R, t);
		cam->setLensDistortion(dist);
		cams.push_back(cam);
		Image im(w, h), mk(w, h);
		rd(f, im.rgba.data(), im.rgba.size());
		std::vector<uint8_t> m(static_cast<size_t>(w)*h);
		rd(f, m.data(), m.size());
		for (size_t k = 0; k < m.size(); ++k) if (!m[k]) { mk.rgba[4*k] = mk.rgba[4*k + 1] = mk.rgba[4*k + 2] = 0; }
		imgs.push_back(im);
		masks.push_back(mk);
	}
	fclose(f);
	TwoViewStereo tv(cams[0], imgs[0], masks[0], cams[1], imgs[1], masks[1], dh[0], dh[1], hdr[3], dh[2]);
	tv.params().window_radius = hdr[4];
	tv.params().weight_kind = hdr[5];
	const int flags = atoi(argv[3]);
	tv.setKeepWtaOutputs(flags);
	if (tv.keepWtaOutputs() != flags) { fprintf(stderr, "keepWtaOutputs\n"); return 3; }
	if (argc > 4 && !strcmp(argv[4], "mrf")) tv.setUseMRF(true);
	tv.computeDepthMaps();
	if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
	FILE *o = fopen(argv[2], "wb");
	if (!o) { perror(argv[2]); return 2; }
	fwrite(tv.leftDepths().data(), sizeof(double), tv.leftDepths().size(), o);
	fwrite(tv.rightDepths().data(), sizeof(double), tv.rightDepths().size(), o);
	const int32_t counts[8] = {
		static_cast<int32_t>(tv.leftWinners().size()), static_cast<int32_t>(tv.leftRunnersUp().size()),
		static_cast<int32_t>(tv.leftMinCosts().size()), static_cast<int32_t>(tv.leftSecondCosts().size()),
		static_cast<int32_t>(tv.rightWinners().size()), static_cast<int32_t>(tv.rightRunnersUp().size()),
		static_cast<int32_t>(tv.rightMinCosts().size()), static_cast<int32_t>(tv.rightSecondCosts().size()) };
	fwrite(counts, sizeof(int32_t), 8, o);
	wr(o, tv.leftWinners()); wr(o, tv.leftRunnersUp()); wr(o, tv.leftMinCosts()); wr(o, tv.leftSecondCosts());
	wr(o, tv.rightWinners()); wr(o, tv.rightRunnersUp()); wr(o, tv.rightMinCosts()); wr(o, tv.rightSecondCosts());
	fclose(o);
	return 0;
}
