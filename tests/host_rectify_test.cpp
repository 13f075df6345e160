// host_rectify_test.cpp -- the Qt-free host class TwoViewStereo with rectification (setRectify):
//   host_rectify_test never in.bin out.bin   computeDepthMaps() of an object on which setRectify was never called
//   host_rectify_test off   in.bin out.bin   setRectify(false); computeDepthMaps()
//   host_rectify_test on    in.bin out.bin   setRectify(true) into (w + 16) x (h - 8) rectified views; computeDepthMaps()
// in.bin / out.bin: the formats of host_api_test.cpp (two views with masks).  `on` checks here that the depth maps have the
// size of the views handed in and the rectified products the size asked for; tests/test_gpu_rectify.py checks the maps.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "host_rectify_test: %s does not hold (line %d)\n", #cond, __LINE__); return 4; } } while (0)

int main(int argc, char **argv) {
	if (argc != 4) { fprintf(stderr, "usage: %s never|off|on in.bin out.bin\n", argv[0]); return 2; }
	const std::string mode = argv[1];
	if (mode != "never" && mode != "off" && mode != "on") { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) { perror(argv[2]); return 2; }
	int32_t hdr[6];
	double dh[4];
	rd(f, hdr, 6); rd(f, dh, 4);
	const int nv = hdr[0], w = hdr[1], h = hdr[2];
	if (nv != 2) { fprintf(stderr, "two views expected\n"); return 2; }
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
		Image mk(w, h);
		std::vector<uint8_t> m(static_cast<size_t>(w)*h);
		rd(f, m.data(), m.size());
		for (size_t k = 0; k < m.size(); ++k) if (!m[k]) { mk.rgba[4*k] = mk.rgba[4*k + 1] = mk.rgba[4*k + 2] = 0; }
		masks.push_back(mk);
	}
	fclose(f);
	TwoViewStereo tv(cams[0], imgs[0], masks[0], cams[1], imgs[1], masks[1], dh[0], dh[1], hdr[3], dh[2]);
	tv.params().window_radius = hdr[4];
	tv.params().weight_kind = hdr[5];
	EXPECT(!tv.rectify());                                   // off by default
	const int ow = w + 16, oh = h - 8;
	if (mode == "off") tv.setRectify(false);
	if (mode == "on") {
		tv.setRectify(true);
		tv.rectifyParams().out_w = ow;
		tv.rectifyParams().out_h = oh;
		tv.setKeepWtaOutputs(SRH_WTA_WINNERS);
	}
	tv.computeDepthMaps();
	if (!tv.lastError().empty()) { fprintf(stderr, "error: %s\n", tv.lastError().c_str()); return 3; }
	const size_t n = static_cast<size_t>(w)*h, nr = static_cast<size_t>(ow)*oh;
	EXPECT(tv.leftDepths().size() == n && tv.rightDepths().size() == n);
	EXPECT(tv.leftDepthMap().w == w && tv.leftDepthMap().h == h);
	if (mode == "on") {
		EXPECT(tv.rectify() && tv.rectified());
		EXPECT(tv.rectifiedLeftDepths().size() == nr && tv.rectifiedRightDepths().size() == nr);
		EXPECT(tv.rectifiedLeftImage().w == ow && tv.rectifiedLeftImage().h == oh);
		EXPECT(tv.rectifiedRightImage().w == ow && tv.rectifiedRightImage().h == oh);
		EXPECT(tv.rectifiedLeftMaskBytes().size() == nr);
		EXPECT(tv.leftWinners().size() == 2*nr);             // the WTA by-products: rectified coordinates
		const srh_camera &ra = tv.rectifiedCamera(true), &rb = tv.rectifiedCamera(false);
		double fx_bx = 0;
		EXPECT(!ra.is_distorted && !rb.is_distorted && srh_twoview_row_aligned(&ra, &rb, &fx_bx) == 1);
		EXPECT(tv.rectifyInfo().white_a > 0 && tv.rectifyInfo().white_b > 0 && tv.rectifyInfo().fx_bx == fx_bx);
		size_t finite = 0;
		for (size_t i = 0; i < nr; ++i) finite += std::isfinite(tv.rectifiedLeftDepths()[i]) ? 1 : 0;
		EXPECT(finite > 0);
	} else {
		EXPECT(!tv.rectified() && tv.rectifiedLeftDepths().empty() && tv.rectifiedLeftImage().isNull());
	}
	FILE *o = fopen(argv[3], "wb");
	if (!o) { perror(argv[3]); return 2; }
	fwrite(tv.leftDepths().data(), sizeof(double), n, o);
	fwrite(tv.rightDepths().data(), sizeof(double), n, o);
	const int32_t ns = 0;
	fwrite(&ns, sizeof(ns), 1, o);
	fclose(o);
	return 0;
}
