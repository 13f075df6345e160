// host_fuse_test.cpp -- the Qt-free MultiViewStereo (stereoreconstruction_amd/host) fusing the depth maps of its run into
// one oriented cloud (fusedPointCloud, fuseParams, the outputPLYFile overload with normals):
//   host_fuse_test in.bin out.bin [min_views]
// in.bin: the format of host_api_test.cpp (MultiViewStereo: masks in the images' alpha).  out.bin: per view double
// depth[w*h]; int32 n; then n records of {double p[3], n[3]; uint8 rgb[3], nviews, flags; int32 view, pixel} packed field by
// field.  out.bin.fused.ply: the cloud through the new overload; out.bin.view0.ply: the first view's own cloud through the
// old one.  tests/test_gpu_fuse_host.py builds the program (without a device too) and checks its outputs against the C-ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "multiviewstereo.hpp"

template <class T> static void rd(FILE *f, T *p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv) {
	if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin [min_views]\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
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
	m->params().window_radius = hdr[4]; m->params().weight_kind = hdr[5];
	const srh_fuse_params &d = m->fuseParams();
	if (d.dist_threshold != 0 || d.normal_depth_gap != 0 || d.min_views != 2 || d.flags != 0) { fprintf(stderr, "fuseParams defaults\n"); return 4; }
	if (argc > 3) m->fuseParams().min_views = atoi(argv[3]);
	m->initialize(cams, imgs, dh[0], dh[1], hdr[3], dh[3], dh[2]);
	m->run();
	if (!m->lastError().empty()) { fprintf(stderr, "run: %s\n", m->lastError().c_str()); return 3; }
	const std::vector<FusedPoint> cloud = m->fusedPointCloud();
	if (!m->lastError().empty()) { fprintf(stderr, "fuse: %s\n", m->lastError().c_str()); return 3; }
	outputPLYFile(std::string(argv[2]) + ".fused.ply", cloud);
	const std::vector<PLYPoint> own = m->pointCloud(cams[0]);
	if (!m->lastError().empty()) { fprintf(stderr, "cloud: %s\n", m->lastError().c_str()); return 3; }
	outputPLYFile(std::string(argv[2]) + ".view0.ply", own);

	FILE *o = fopen(argv[2], "wb");
	if (!o) { perror(argv[2]); return 2; }
	for (int v = 0; v < nv; ++v) fwrite(m->depths(cams[v])->data(), sizeof(double), m->depths(cams[v])->size(), o);
	const int32_t n = static_cast<int32_t>(cloud.size());
	fwrite(&n, sizeof(n), 1, o);
	for (const FusedPoint &q : cloud) {
		fwrite(q.p, sizeof(double), 3, o); fwrite(q.n, sizeof(double), 3, o);
		fwrite(q.rgb, 1, 3, o); fwrite(&q.nviews, 1, 1, o); fwrite(&q.flags, 1, 1, o);
		const int32_t src[2] = { q.view, q.pixel };
		fwrite(src, sizeof(int32_t), 2, o);
	}
	fclose(o);
	return 0;
}
