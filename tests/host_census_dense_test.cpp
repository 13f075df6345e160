// host_census_dense_test.cpp -- the Qt-free TwoViewStereo (stereoreconstruction_amd/host) with the census matching cost and
// setCensusDense:
//   host_census_dense_test in.bin out.bin on      setCostFunction(SRH_COST_CENSUS); setCensusDense(on); computeDepthMaps()
// in.bin / out.bin: the formats of host_api_test.cpp (two views, with masks); tests/test_gpu_census_dense.py checks that the
// maps do not depend on the switch, tests/test_census_dense_host.py compiles it without a device.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv) {
	if (argc < 4) { fprintf(stderr, "usage: %s in.bin out.bin on\n", argv[0]); return 2; }
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
	std::vector<int32_t> steps;
	tv.progressUpdate = [&](int s) { steps.push_back(s); };
	tv.setCostFunction(SRH_COST_CENSUS);
	tv.setCensusDense(atoi(argv[3]));
	if (tv.censusDense() != atoi(argv[3])) { fprintf(stderr, "censusDense\n"); return 3; }
	tv.computeDepthMaps();
	if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
	FILE *o = fopen(argv[2], "wb");
	if (!o) { perror(argv[2]); return 2; }
	fwrite(tv.leftDepths().data(), sizeof(double), tv.leftDepths().size(), o);
	fwrite(tv.rightDepths().data(), sizeof(double), tv.rightDepths().size(), o);
	const int32_t ns = static_cast<int32_t>(steps.size());
	fwrite(&ns, sizeof(ns), 1, o);
	fwrite(steps.data(), sizeof(int32_t), steps.size(), o);
	fclose(o);
	return 0;
}
