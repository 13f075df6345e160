// host_twoview_sgm_test.cpp -- the Qt-free TwoViewStereo (stereoreconstruction_amd/host) with its semi-global aggregation:
//   host_twoview_sgm_test defaults                          no device needed: the switch is off, sgmParams() holds the
//                                                           defaults, setUseSGM and setUseMRF switch each other off,
//                                                           numSteps() is 8; prints the parameters
//   host_twoview_sgm_test compute in.bin out.bin sgm cost   setUseSGM(sgm); setCostFunction(cost); computeDepthMaps()
// in.bin: the format of host_api_test.cpp (two views, with masks).  out.bin: both maps, the progress steps (count, values),
// then per map (paths, energy) as doubles and the four sizes of the WTA by-product vectors of the left map.
// tests/test_gpu_twoview_sgm.py checks it against the C-ABI; tests/test_twoview_sgm_host.py compiles it and runs `defaults`
// without a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv) {
	if (argc >= 2 && std::string(argv[1]) == "defaults") {
		double K[9] = { 100, 0, 4, 0, 100, 3, 0, 0, 1 }, R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 };
		CameraPtr a(new Camera("0", "a")), b(new Camera("1", "b"));
		a->set(K, R, t); b->set(K, R, t);
		TwoViewStereo tv(a, Image(8, 6), Image(), b, Image(8, 6), Image(), 1.0, 2.0, 16);
		if (tv.useSGM() || tv.useMRF()) return 3;
		tv.setUseSGM(true);
		if (!tv.useSGM() || tv.useMRF() || tv.numSteps() != 8 || tv.sgmInfo(true).paths != 0 || tv.sgmInfo(false).paths != 0) return 3;
		tv.setUseMRF(true);                                         // the last call wins
		if (tv.useSGM() || !tv.useMRF()) return 4;
		tv.setUseSGM(true);
		if (!tv.useSGM() || tv.useMRF()) return 4;
		tv.setUseSGM(false);
		if (tv.useSGM() || tv.useMRF()) return 4;
		const srh_twoview_sgm_params &m = tv.sgmParams();
		printf("%d %g %g %d\n", (int)m.smooth_exp, m.smooth_max, m.lambda, (int)m.path_mask);
		return 0;
	}
	if (argc < 6 || std::string(argv[1]) != "compute") { fprintf(stderr, "usage: %s defaults | compute in.bin out.bin sgm cost\n", argv[0]); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) { perror(argv[2]); return 2; }
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
	std::vector<int32_t> steps;
	tv.progressUpdate = [&](int s) { steps.push_back(s); };
	tv.setUseSGM(atoi(argv[4]) != 0);
	tv.setCostFunction(atoi(argv[5]));
	tv.computeDepthMaps();
	if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
	FILE *o = fopen(argv[3], "wb");
	if (!o) { perror(argv[3]); return 2; }
	fwrite(tv.leftDepths().data(), sizeof(double), tv.leftDepths().size(), o);
	fwrite(tv.rightDepths().data(), sizeof(double), tv.rightDepths().size(), o);
	const int32_t ns = static_cast<int32_t>(steps.size());
	fwrite(&ns, sizeof(ns), 1, o);
	fwrite(steps.data(), sizeof(int32_t), steps.size(), o);
	for (int k = 0; k < 2; ++k) {
		const srh_sgm_info &i = tv.sgmInfo(k == 0);
		const double rec[2] = { (double)i.paths, i.energy };
		fwrite(rec, sizeof(double), 2, o);
	}
	const double sizes[4] = { (double)tv.leftWinners().size(), (double)tv.leftRunnersUp().size(), (double)tv.leftMinCosts().size(),
	                          (double)tv.leftSecondCosts().size() };
	fwrite(sizes, sizeof(double), 4, o);
	fclose(o);
	return 0;
}
