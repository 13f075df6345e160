// host_scale_test.cpp -- the host classes' forms that take images at file resolution and scale them on the device
// (MultiViewStereo::initialize with an ImageDecoder, TwoViewStereo's ScaleOnDevice constructor) against the forms that take
// ALREADY SCALED images, fed the output of tests/qt_scale_ref.py: the same images, the same masks, the same depth maps, bit
// for bit.  Inputs are written by tests/test_scale_host.py.
//
//   host_scale_test in.bin        exit 0 and "OK" when everything agrees
//
// in.bin: int32 n (2), sw, sh, hasAlpha, w, h, mw, mh, D; double scale, zmin, zmax, crossCheck;
//         per view: double K[9], R[9], t[3]; uint8 src[sw*sh*4] (file resolution); uint8 smooth[w*h*4], fast[mw*mh*4] (the
//         restatement's two scalings of src); uint8 msrc[sw*sh*4] (a mask image at file resolution), msmooth[w*h*4] (its
//         smooth scaling by the restatement)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "multiviewstereo.hpp"
#include "twoviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

static Image readImage(FILE *f, int w, int h, bool hasAlpha = true) {
	Image im(w, h);
	rd(f, im.rgba.data(), im.rgba.size());
	im.hasAlpha = hasAlpha;
	return im;
}

static int fail(const char *what) { fprintf(stderr, "MISMATCH: %s\n", what); return 1; }

static bool sameBits(const std::vector<double> &a, const std::vector<double> &b) {
	return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size()*sizeof(double)));
}

int main(int argc, char **argv) {
	if (argc != 2) { fprintf(stderr, "usage: %s in.bin\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	int32_t hdr[9]; double dh[4];
	rd(f, hdr, 9); rd(f, dh, 4);
	const int n = hdr[0], sw = hdr[1], sh = hdr[2], w = hdr[4], h = hdr[5], mw = hdr[6], mh = hdr[7], D = hdr[8];
	const bool hasAlpha = hdr[3] != 0;
	const double scale = dh[0], zmin = dh[1], zmax = dh[2], cc = dh[3];
	if (n != 2) return 2;
	std::vector<CameraPtr> cams;
	std::vector<Image> src, smooth, fast, msrc, msmooth;
	for (int v = 0; v < n; ++v) {
		double K[9], R[9], t[3];
		rd(f, K, 9); rd(f, R, 9); rd(f, t, 3);
		CameraPtr c(new Camera(std::to_string(v), "cam" + std::to_string(v)));
		c->set(K, R, t);
		cams.push_back(c);
		src.push_back(readImage(f, sw, sh, hasAlpha));
		smooth.push_back(readImage(f, w, h));
		fast.push_back(readImage(f, mw, mh));
		msrc.push_back(readImage(f, sw, sh, false));
		msmooth.push_back(readImage(f, w, h));
	}
	fclose(f);

	// ---- MultiViewStereo: ImageDecoder (the library scales) against ImageLoader (the caller has scaled)
	ProjectPtr prj(new Project());
	ImageSetPtr set(new ImageSet("set"));
	for (int v = 0; v < n; ++v) set->addImageForCamera(cams[v], ProjectImagePtr(new ProjectImage(std::to_string(v))));
	MultiViewStereo::ImageDecoder decode = [&](const std::string &file, Image &image) { image = src[atoi(file.c_str())]; return true; };
	MultiViewStereo::ImageLoader load = [&](const std::string &file, double, Image &image, Image &maskSource) {
		image = smooth[atoi(file.c_str())];
		if (hasAlpha) maskSource = fast[atoi(file.c_str())];
		return true;
	};
	MultiViewStereo a, b;
	if (!a.lastError().empty()) { fprintf(stderr, "ctor: %s\n", a.lastError().c_str()); return 3; }
	a.initialize(prj, set, cams, zmin, zmax, D, cc, scale, decode);
	b.initialize(prj, set, cams, zmin, zmax, D, cc, scale, load);
	if (!a.lastError().empty()) { fprintf(stderr, "initialize: %s\n", a.lastError().c_str()); return 3; }
	for (int v = 0; v < n; ++v) {
		const Image *ia = a.image(cams[v]), *ib = b.image(cams[v]);
		if (!ia || !ib) return fail("a view was skipped");
		if (ia->w != ib->w || ia->h != ib->h || ia->rgba != ib->rgba) return fail("MultiViewStereo image");
		if (*a.mask(cams[v]) != *b.mask(cams[v])) return fail("MultiViewStereo mask");
	}
	a.run(); b.run();
	if (!a.lastError().empty() || !b.lastError().empty()) { fprintf(stderr, "run: %s %s\n", a.lastError().c_str(), b.lastError().c_str()); return 3; }
	size_t finite = 0;
	for (int v = 0; v < n; ++v) {
		if (!sameBits(*a.depths(cams[v]), *b.depths(cams[v]))) return fail("MultiViewStereo depth map");
		for (double d : *a.depths(cams[v])) finite += d == d && d - d == 0;
	}
	// a view the library does not scale is skipped with the error kept
	MultiViewStereo c;
	c.initialize(prj, set, cams, zmin, zmax, D, cc, 1.5, decode);
	if (c.image(cams[0]) || c.lastError().empty()) return fail("up-scaling was not refused");

	// ---- TwoViewStereo: ScaleOnDevice against the constructor that takes scaled images and mask images
	TwoViewStereo ta(TwoViewStereo::ScaleOnDevice(), cams[0], src[0], msrc[0], cams[1], src[1], Image(), zmin, zmax, D, scale);
	TwoViewStereo tb(cams[0], smooth[0], msmooth[0], cams[1], smooth[1], Image(), zmin, zmax, D, scale);
	if (!ta.lastError().empty()) { fprintf(stderr, "TwoViewStereo: %s\n", ta.lastError().c_str()); return 3; }
	if (ta.leftImage().rgba != tb.leftImage().rgba || ta.rightImage().rgba != tb.rightImage().rgba) return fail("TwoViewStereo image");
	if (ta.leftMaskBytes() != tb.leftMaskBytes() || ta.rightMaskBytes() != tb.rightMaskBytes()) return fail("TwoViewStereo mask");
	ta.computeDepthMaps(); tb.computeDepthMaps();
	if (!ta.lastError().empty() || !tb.lastError().empty()) { fprintf(stderr, "compute: %s %s\n", ta.lastError().c_str(), tb.lastError().c_str()); return 3; }
	if (!sameBits(ta.leftDepths(), tb.leftDepths()) || !sameBits(ta.rightDepths(), tb.rightDepths())) return fail("TwoViewStereo depth map");
	size_t masked = 0;
	for (uint8_t m : ta.leftMaskBytes()) masked += m;
	printf("OK mvs_finite %zu twoview_left_white %zu of %zu\n", finite, masked, ta.leftMaskBytes().size());
	return 0;
}
