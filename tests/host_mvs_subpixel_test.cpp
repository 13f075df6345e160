// host_mvs_subpixel_test.cpp -- the Qt-free MultiViewStereo (stereoreconstruction_amd/host) with its sub-pixel stage:
//   host_mvs_subpixel_test defaults                          no device needed: the stage is off, setSubpixel / subpixel() /
//                                                            subpixelInfo(view) exist, numSteps() stays 2*views
//   host_mvs_subpixel_test compute in.bin out.bin on [mode]  setSubpixel(on); mode "sgm" / "mrf": setUseSGM / setUseMRF; run()
// in.bin: the "mvs" format of host_api_test.cpp (the mask is the image's alpha).  out.bin: every view's map, the progress
// steps (count, values), then per view the 8 int64 of subpixelInfo (n_class[6], n_moved, n_fallback).
// Built by `make -C stereoreconstruction_amd/host mvs_subpixel_test TESTBIN=<dir>`; tests/test_gpu_mvs_subpixel.py checks
// it against the C-ABI, tests/test_mvs_subpixel_ref.py builds it and runs `defaults` without a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "multiviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv) {
	if (argc >= 2 && std::string(argv[1]) == "defaults") {
		double K[9] = { 100, 0, 4, 0, 100, 3, 0, 0, 1 }, R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 };
		std::vector<CameraPtr> cams;
		std::vector<Image> imgs;
		for (int v = 0; v < 3; ++v) {
			CameraPtr c(new Camera(std::to_string(v), "cam" + std::to_string(v)));
			c->set(K, R, t);
			cams.push_back(c);
			imgs.push_back(Image(8, 6));
		}
		MultiViewStereo m;
		m.initialize(cams, imgs, 1.0, 2.0, 16, 0.01);
		if (m.subpixel()) return 3;
		m.setSubpixel(true);
		if (!m.subpixel() || m.numSteps() != 6 || m.useMRF() || m.useSGM()) return 3;
		const srh_mvs_subpixel_info i = m.subpixelInfo(cams[0]);
		for (int k = 0; k < 6; ++k) if (i.n_class[k] != 0) return 4;
		if (i.n_moved != 0 || i.n_fallback != 0 || m.subpixelInfo(CameraPtr(new Camera("x"))).n_moved != 0) return 4;
		m.setSubpixel(false);
		if (m.subpixel()) return 4;
		printf("%d\n", (int)SRH_SUBPX_NO_WINNER);
		return 0;
	}
	if (argc < 5 || std::string(argv[1]) != "compute") { fprintf(stderr, "usage: %s defaults | compute in.bin out.bin on [sgm|mrf]\n", argv[0]); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) { perror(argv[2]); return 2; }
	int32_t hdr[6];
	double dh[4];
	rd(f, hdr, 6); rd(f, dh, 4);
	const int nv = hdr[0], w = hdr[1], h = hdr[2];
	std::vector<CameraPtr> cams;
	std::vector<Image> imgs;
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
	}
	fclose(f);
	std::shared_ptr<MultiViewStereo> m(new MultiViewStereo());
	if (!m->lastError().empty()) { fprintf(stderr, "ctor: %s\n", m->lastError().c_str()); return 3; }
	m->params().window_radius = hdr[4];
	m->params().weight_kind = hdr[5];
	m->setSubpixel(atoi(argv[4]) != 0);
	if (argc > 5 && std::string(argv[5]) == "sgm") m->setUseSGM(true);
	if (argc > 5 && std::string(argv[5]) == "mrf") m->setUseMRF(true);
	m->initialize(cams, imgs, dh[0], dh[1], hdr[3], dh[3], dh[2]);
	std::vector<int32_t> steps;
	m->progressUpdate = [&](int s) { steps.push_back(s); };
	if (m->numSteps() != 2*nv) return 4;
	m->run();
	if (!m->lastError().empty()) { fprintf(stderr, "run: %s\n", m->lastError().c_str()); return 3; }
	FILE *o = fopen(argv[3], "wb");
	if (!o) { perror(argv[3]); return 2; }
	for (int v = 0; v < nv; ++v) fwrite(m->depths(cams[v])->data(), sizeof(double), m->depths(cams[v])->size(), o);
	const int32_t ns = static_cast<int32_t>(steps.size());
	fwrite(&ns, sizeof(ns), 1, o);
	fwrite(steps.data(), sizeof(int32_t), steps.size(), o);
	for (int v = 0; v < nv; ++v) {
		const srh_mvs_subpixel_info i = m->subpixelInfo(cams[v]);
		int64_t rec[8];
		for (int k = 0; k < 6; ++k) rec[k] = i.n_class[k];
		rec[6] = i.n_moved; rec[7] = i.n_fallback;
		fwrite(rec, sizeof(int64_t), 8, o);
	}
	fclose(o);
	return 0;
}
