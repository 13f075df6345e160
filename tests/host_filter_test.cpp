// host_filter_test.cpp -- the Qt-free TwoViewStereo (stereoreconstruction_amd/host) with hole filling, driven two ways:
//   host_filter_test compute in.bin out.bin flags   setFilterInvalid(flags); computeDepthMaps()
//   host_filter_test stages  in.bin out.bin flags   a subclass runs computeCostVolumes, crossCheck, filterInvalidPixels
// in.bin / out.bin: the formats of host_api_test.cpp (two views, with masks); tests/test_gpu_filter.py checks them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

class StagedTwoView : public TwoViewStereo {
public:
	using TwoViewStereo::TwoViewStereo;
	void runStages(CameraPtr l, CameraPtr r) {
		computeCostVolumes(l, r);
		crossCheck(l, r);
		filterInvalidPixels();
	}
};

int main(int argc, char **argv) {
	if (argc != 5) { fprintf(stderr, "usage: %s compute|stages in.bin out.bin flags\n", argv[0]); return 2; }
	const std::string mode = argv[1];
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
	StagedTwoView tv(cams[0], imgs[0], masks[0], cams[1], imgs[1], masks[1], dh[0], dh[1], hdr[3], dh[2]);
	tv.params().window_radius = hdr[4];
	tv.params().weight_kind = hdr[5];
	tv.setFilterInvalid(atoi(argv[4]));
	std::vector<int32_t> steps;
	tv.progressUpdate = [&](int s) { steps.push_back(s); };
	if (mode == "compute") tv.computeDepthMaps();
	else if (mode == "stages") tv.runStages(cams[0], cams[1]);
	else { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
	if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
	FILE *o = fopen(argv[3], "wb");
	if (!o) { perror(argv[3]); return 2; }
	fwrite(tv.leftDepths().data(), sizeof(double), tv.leftDepths().size(), o);
	fwrite(tv.rightDepths().data(), sizeof(double), tv.rightDepths().size(), o);
	const int32_t ns = static_cast<int32_t>(steps.size());
	fwrite(&ns, sizeof(ns), 1, o);
	fwrite(steps.data(), sizeof(int32_t), steps.size(), o);
	fclose(o);
	return 0;
}
