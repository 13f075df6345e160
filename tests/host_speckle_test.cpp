// host_speckle_test.cpp -- the Qt-free host classes (stereoreconstruction_amd/host) with the speckle filter:
//   host_speckle_test twoview in.bin out.bin minSize diffSteps   TwoViewStereo: setSpeckleFilter(minSize, diffSteps); computeDepthMaps()
//   host_speckle_test stages  in.bin out.bin minSize diffSteps   a subclass runs computeCostVolumes, crossCheck, filterSpeckles
//   host_speckle_test mvs     in.bin out.bin minSize maxDiff     MultiViewStereo: setSpeckleFilter(minSize, maxDiff); run()
// in.bin / out.bin: the formats of host_api_test.cpp (twoview / stages: two views with masks; mvs: the masks in the images'
// alpha); minSize 0 is the run without the filter.  tests/test_gpu_speckle_host.py checks the maps.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "multiviewstereo.hpp"
#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

class StagedTwoView : public TwoViewStereo {
public:
	using TwoViewStereo::TwoViewStereo;
	void runStages(CameraPtr l, CameraPtr r) {
		computeCostVolumes(l, r);
		crossCheck(l, r);
		filterSpeckles();
	}
};

int main(int argc, char **argv) {
	if (argc != 6) { fprintf(stderr, "usage: %s twoview|stages|mvs in.bin out.bin minSize diffSteps|maxDiff\n", argv[0]); return 2; }
	const std::string mode = argv[1];
	const bool mvs = mode == "mvs";
	if (!mvs && mode != "twoview" && mode != "stages") { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) { perror(argv[2]); return 2; }
	int32_t hdr[6];
	double dh[4];
	rd(f, hdr, 6); rd(f, dh, 4);
	const int nv = hdr[0], w = hdr[1], h = hdr[2];
	if (!mvs && nv != 2) { fprintf(stderr, "two views expected\n"); return 2; }
	std::vector<CameraPtr> cams;
	std::vector<Image> imgs, masks;
	for (int v = 0; v < nv; ++v) {
		double K[9], R[9], t[3]; LensDistortions dist;
		rd(f, K, 9); rd(f, R, 9); rd(f, t, 3); rd(f, dist.data(), 5);
		CameraPtr cam(new Camera(std::to_string(v), "cam" + std::to_string(v)));
		cam->set(K, R, t);
		cam->setLensDistortion(dist);
		cams.push_back(cam);
		Image im(w, h);
		rd(f, im.rgba.data(), im.rgba.size());
		imgs.push_back(im);
		if (!mvs) {
			Image mk(w, h);
			std::vector<uint8_t> m(static_cast<size_t>(w)*h);
			rd(f, m.data(), m.size());
			for (size_t k = 0; k < m.size(); ++k) if (!m[k]) { mk.rgba[4*k] = mk.rgba[4*k + 1] = mk.rgba[4*k + 2] = 0; }
			masks.push_back(mk);
		}
	}
	fclose(f);
	const int minSize = atoi(argv[4]);
	std::vector<int32_t> steps;
	std::vector<std::vector<double> > out;
	if (!mvs) {
		StagedTwoView tv(cams[0], imgs[0], masks[0], cams[1], imgs[1], masks[1], dh[0], dh[1], hdr[3], dh[2]);
		tv.params().window_radius = hdr[4];
		tv.params().weight_kind = hdr[5];
		tv.setSpeckleFilter(minSize, atoi(argv[5]));
		if (tv.speckleFilter() != minSize || tv.numSteps() != 8) return 4;
		tv.progressUpdate = [&](int s) { steps.push_back(s); };
		if (mode == "twoview") tv.computeDepthMaps();
		else tv.runStages(cams[0], cams[1]);
		if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
		out.push_back(tv.leftDepths()); out.push_back(tv.rightDepths());
	} else {
		std::shared_ptr<MultiViewStereo> m(new MultiViewStereo());
		if (!m->lastError().empty()) { fprintf(stderr, "ctor: %s\n", m->lastError().c_str()); return 3; }
		m->params().window_radius = hdr[4]; m->params().weight_kind = hdr[5];
		m->initialize(cams, imgs, dh[0], dh[1], hdr[3], dh[3], dh[2]);
		m->setSpeckleFilter(minSize, atof(argv[5]));
		if (m->speckleFilter() != minSize || m->numSteps() != 2*nv) return 4;
		m->progressUpdate = [&](int s) { steps.push_back(s); };
		m->run();
		if (!m->lastError().empty()) { fprintf(stderr, "run: %s\n", m->lastError().c_str()); return 3; }
		for (int v = 0; v < nv; ++v) out.push_back(*m->depths(cams[v]));
	}
	FILE *o = fopen(argv[3], "wb");
	if (!o) { perror(argv[3]); return 2; }
	for (size_t v = 0; v < out.size(); ++v) fwrite(out[v].data(), sizeof(double), out[v].size(), o);
	const int32_t ns = static_cast<int32_t>(steps.size());
	fwrite(&ns, sizeof(ns), 1, o);
	fwrite(steps.data(), sizeof(int32_t), steps.size(), o);
	fclose(o);
	return 0;
}
