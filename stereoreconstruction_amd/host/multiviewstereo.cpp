// multiviewstereo.cpp -- host side of MultiViewStereo above the C-ABI (reference:
// stereo/multiviewstereo.cpp:193-475).  Sequencing and bookkeeping only.
#include "multiviewstereo.hpp"

#include <cmath>
#include <fstream>
#include <limits>

void outputPLYFile(const std::string &path, const std::vector<PLYPoint> &points) {
	std::ofstream lout(path.c_str());
	lout << "ply\n" << "format ascii 1.0\n" << "element vertex " << points.size() << "\n"
	     << "property float x\n" << "property float y\n" << "property float z\n"
	     << "property uchar diffuse_red\n" << "property uchar diffuse_green\n" << "property uchar diffuse_blue\n"
	     << "end_header\n";
	for (size_t i = 0; i < points.size(); ++i) {
		const PLYPoint &pp = points[i];
		lout << pp.p[0] << ' ' << pp.p[1] << ' ' << pp.p[2] << ' '
		     << static_cast<int>(pp.rgb[0]) << ' ' << static_cast<int>(pp.rgb[1]) << ' ' << static_cast<int>(pp.rgb[2]) << '\n';
	}
}

void outputPLYFile(const std::string &path, const std::vector<FusedPoint> &points) {
	std::ofstream lout(path.c_str());
	lout << "ply\n" << "format ascii 1.0\n" << "element vertex " << points.size() << "\n"
	     << "property float x\n" << "property float y\n" << "property float z\n"
	     << "property float nx\n" << "property float ny\n" << "property float nz\n"
	     << "property uchar diffuse_red\n" << "property uchar diffuse_green\n" << "property uchar diffuse_blue\n"
	     << "end_header\n";
	for (size_t i = 0; i < points.size(); ++i) {
		const FusedPoint &pp = points[i];
		lout << pp.p[0] << ' ' << pp.p[1] << ' ' << pp.p[2] << ' ' << pp.n[0] << ' ' << pp.n[1] << ' ' << pp.n[2] << ' '
		     << static_cast<int>(pp.rgb[0]) << ' ' << static_cast<int>(pp.rgb[1]) << ' ' << static_cast<int>(pp.rgb[2]) << '\n';
	}
}

MultiViewStereo::MultiViewStereo(int deviceOrdinal)
	: minDepth(0), maxDepth(0), crossCheckThreshold(0), imageScale(1), numDepthLevels(0), ctx_(nullptr)
{
	srh_params_mvs_defaults(&params_);
	srh_mrf_params_defaults(&mrfParams_);
	srh_mvs_sgm_params_defaults(&sgmParams_);
	srh_fuse_params_defaults(&fuseParams_);
	if (srh_create(deviceOrdinal, &ctx_) != SRH_OK) { error_ = srh_last_error(); ctx_ = nullptr; }
}

MultiViewStereo::~MultiViewStereo() { if (ctx_) srh_destroy(ctx_); }

void MultiViewStereo::initialize(const std::vector<CameraPtr> &views_, const std::vector<Image> &images_,
                                 double minDepth_, double maxDepth_, int numDepthLevels_,
                                 double crossCheckThreshold_, double imageScale_)
{
	// multiviewstereo.cpp:193-247
	minDepth = minDepth_; maxDepth = maxDepth_; numDepthLevels = numDepthLevels_;
	crossCheckThreshold = crossCheckThreshold_; imageScale = imageScale_;
	views.clear(); images.clear(); masks.clear(); results.clear(); computedDepths.clear();
	const double NaN = std::numeric_limits<double>::quiet_NaN();
	for (size_t i = 0; i < views_.size() && i < images_.size(); ++i) {
		if (!views_[i] || images_[i].isNull()) continue;
		const Image &im = images_[i];
		images.push_back(im);
		std::vector<uint8_t> m(static_cast<size_t>(im.w)*im.h);
		for (size_t k = 0; k < m.size(); ++k) m[k] = im.rgba[k*4 + 3] == 255 ? 1 : 0;   // not fully opaque => ignored
		masks.push_back(m);
		results.push_back(Image(im.w, im.h));
		computedDepths.push_back(DepthMap(static_cast<size_t>(im.w)*im.h, NaN));
		views.push_back(views_[i]);
	}
	neighbours.assign(views.size(), std::vector<int>());
	sgmInfos_.assign(views.size(), srh_sgm_info());
	subpixelInfos_.clear();
}

void MultiViewStereo::initialize(ProjectPtr project_, ImageSetPtr imageSet__, const std::vector<CameraPtr> &views_,
                                 double minDepth_, double maxDepth_, int numDepthLevels_,
                                 double crossCheckThreshold_, double imageScale_, const ImageLoader &load)
{
	// multiviewstereo.cpp:193-247 with the file access handed to `load`
	std::vector<CameraPtr> kept;
	std::vector<Image> imgs, maskSrc;
	for (size_t i = 0; i < views_.size(); ++i) if (views_[i] && imageSet__) {
		const ProjectImagePtr pi = imageSet__->defaultImageForCamera(views_[i]);
		Image im, ms;
		if (!pi || !load || !load(pi->file(), imageScale_, im, ms) || im.isNull()) continue;
		kept.push_back(views_[i]); imgs.push_back(im); maskSrc.push_back(ms);
	}
	initialize(kept, imgs, minDepth_, maxDepth_, numDepthLevels_, crossCheckThreshold_, imageScale_);
	project = project_;
	imageSet_ = imageSet__;
	for (size_t v = 0; v < views.size(); ++v) {
		// mask: alpha == 255 on the fast-scaled copy; no alpha channel => WHITE everywhere (:225-237)
		if (maskSrc[v].isNull()) masks[v].assign(masks[v].size(), 1);
		else if (maskSrc[v].w == images[v].w && maskSrc[v].h == images[v].h) masks[v] = maskFromAlpha(maskSrc[v]);
	}
}

void MultiViewStereo::initialize(ProjectPtr project_, ImageSetPtr imageSet__, const std::vector<CameraPtr> &views_,
                                 double minDepth_, double maxDepth_, int numDepthLevels_,
                                 double crossCheckThreshold_, double imageScale_, const ImageDecoder &decode)
{
	// multiviewstereo.cpp:193-247 with the decoding handed to `decode` and both scalings done on the device
	std::vector<CameraPtr> kept;
	std::vector<Image> imgs;
	std::vector<std::vector<uint8_t> > scaledMasks;
	for (size_t i = 0; i < views_.size() && ctx_; ++i) if (views_[i] && imageSet__) {
		const ProjectImagePtr pi = imageSet__->defaultImageForCamera(views_[i]);
		Image src;
		if (!pi || !decode || !decode(pi->file(), src) || src.isNull()) continue;
		const srh_camera cam = views_[i]->snapshot();
		const int slot = static_cast<int>(kept.size());
		if (slot >= SRH_MAX_VIEWS) { error_ = "too many views"; break; }
		int w = 0, h = 0;
		if (srh_view_upload_scaled(ctx_, slot, src.w, src.h, src.rgba.data(), src.hasAlpha ? 1 : 0, nullptr, 0, 0, 0,
		                           imageScale_, SRH_MASK_ALPHA_FAST, &cam) != SRH_OK ||
		    srh_view_size(ctx_, slot, &w, &h) != SRH_OK) { error_ = srh_last_error(); continue; }
		Image im(w, h);
		im.hasAlpha = src.hasAlpha;
		std::vector<uint8_t> m(static_cast<size_t>(w)*h);
		if (srh_view_image_download(ctx_, slot, im.rgba.data(), m.data()) != SRH_OK) { error_ = srh_last_error(); continue; }
		kept.push_back(views_[i]); imgs.push_back(im); scaledMasks.push_back(m);
	}
	initialize(kept, imgs, minDepth_, maxDepth_, numDepthLevels_, crossCheckThreshold_, imageScale_);
	project = project_;
	imageSet_ = imageSet__;
	masks = scaledMasks;
}

const Image *MultiViewStereo::image(CameraPtr view) const {
	for (size_t v = 0; v < views.size(); ++v) if (views[v] == view) return &images[v];
	return nullptr;
}

const std::vector<uint8_t> *MultiViewStereo::mask(CameraPtr view) const {
	for (size_t v = 0; v < views.size(); ++v) if (views[v] == view) return &masks[v];
	return nullptr;
}

int MultiViewStereo::numSteps() const { return 2*static_cast<int>(views.size()); }

void MultiViewStereo::colorize(size_t v) {
	// runTask "Constructing depth maps" (multiviewstereo.cpp:382-395) + colorFromDepth (:257-276)
	Image &out = results[v];
	for (int y = 0; y < out.h; ++y)
		for (int x = 0; x < out.w; ++x) {
			const size_t i = static_cast<size_t>(y)*out.w + x;
			uint8_t g = 255;
			const double d = computedDepths[v][i];
			if (masks[v][i] == 1 && !std::isnan(d) && !std::isinf(d) && !(d + 1e-5 < minDepth)) {
				double t = (d - minDepth) / (maxDepth - minDepth);
				t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
				g = static_cast<uint8_t>(255*t);
			}
			uint8_t *p = out.pixel(x, y);
			p[0] = p[1] = p[2] = g; p[3] = 255;
		}
}

void MultiViewStereo::runTask() {
	// multiviewstereo.cpp:325-475
	if (!ctx_ || views.empty()) return;               // reference: silent return (":326-327 TODO error")
	const int nv = static_cast<int>(views.size());
	if (nv > SRH_MAX_VIEWS) { error_ = "too many views"; return; }
	params_.min_depth = minDepth; params_.max_depth = maxDepth; params_.num_depth_levels = numDepthLevels;
	params_.image_scale = imageScale; params_.cross_check_threshold = crossCheckThreshold;
	int current_step = 0;

	std::vector<srh_camera> cams(nv);
	for (int v = 0; v < nv; ++v) cams[v] = views[v]->snapshot();
	std::vector<int32_t> neigh(static_cast<size_t>(nv)*params_.num_neighbours, -1), count(nv, 0);
	if (srh_mvs_neighbours(nv, cams.data(), &params_, neigh.data(), count.data()) != SRH_OK) { error_ = srh_last_error(); return; }
	for (int v = 0; v < nv; ++v) {
		neighbours[v].assign(neigh.begin() + static_cast<size_t>(v)*params_.num_neighbours,
		                     neigh.begin() + static_cast<size_t>(v)*params_.num_neighbours + count[v]);
		if (srh_view_upload(ctx_, v, images[v].w, images[v].h, images[v].rgba.data(), masks[v].data(), &cams[v]) != SRH_OK) {
			error_ = srh_last_error(); return;
		}
	}
	srh_set_hooks(ctx_, cancelFlag(), nullptr, nullptr);

	for (int v = 0; v < nv; ++v) {                     // initial stereo estimate, :365-376
		emitProgress(current_step++);
		emitStage("Computing cost volume for camera " + views[v]->name());
		const int32_t *nb = &neigh[static_cast<size_t>(v)*params_.num_neighbours];
		// #ifdef USE_MRF (:610-652): the peaks are kept and the MRF stage of all views runs afterwards, side by side
		// (the views' estimates do not depend on each other: the same results as one view after the other)
		const int rc = useMrf_ || useSgm_ ? srh_mvs_initial_estimate_peaks(ctx_, v, nb, count[v], &params_)
		                                  : srh_mvs_initial_estimate(ctx_, v, nb, count[v], &params_, 0, 0, nullptr);
		if (rc == SRH_E_CANCELLED || isCancelled()) { srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
		if (rc != SRH_OK) { error_ = srh_last_error(); srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
	}
	if (useMrf_) {
		std::vector<int32_t> all(nv);
		for (int v = 0; v < nv; ++v) all[v] = v;
		const int rc = srh_mvs_mrf_estimate_views(ctx_, all.data(), nv, &mrfParams_, nullptr);
		if (rc == SRH_E_CANCELLED || isCancelled()) { srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
		if (rc != SRH_OK) { error_ = srh_last_error(); srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
	}
	if (useSgm_) {                                     // the aggregation where the MRF branch sits: all views side by side
		std::vector<int32_t> all(nv);
		for (int v = 0; v < nv; ++v) all[v] = v;
		sgmInfos_.assign(nv, srh_sgm_info());
		const int rc = srh_mvs_sgm_estimate_views(ctx_, all.data(), nv, &sgmParams_, sgmInfos_.data());
		if (rc == SRH_E_CANCELLED || isCancelled()) { srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
		if (rc != SRH_OK) { error_ = srh_last_error(); srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
	}
	if (subpixel_) {
		// sub-pixel depth (not in the reference): every view's finished map -- the WTA's, the MRF's or the aggregation's --
		// with the neighbour list its estimate used, before anything else reads it (no step of its own)
		subpixelInfos_.assign(nv, srh_mvs_subpixel_info());
		for (int v = 0; v < nv; ++v) {
			const int rc = srh_mvs_view_subpixel(ctx_, v, &neigh[static_cast<size_t>(v)*params_.num_neighbours], count[v], &params_,
			                                     &subpixelInfos_[v], nullptr, nullptr, nullptr, nullptr);
			if (rc == SRH_E_CANCELLED || isCancelled()) { srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
			if (rc != SRH_OK) { error_ = srh_last_error(); srh_set_hooks(ctx_, nullptr, nullptr, nullptr); return; }
		}
	}
	emitStage("Constructing depth maps");
	for (int v = 0; v < nv; ++v) {
		srh_view_depth_download(ctx_, v, computedDepths[v].data());
		colorize(v);
	}

	emitStage("Cross-checking");                       // :427-431, views in order
	std::vector<int32_t> slots(nv);
	for (int v = 0; v < nv; ++v) slots[v] = v;
	bool checked = true;
	for (int v = 0; v < nv; ++v) {
		emitProgress(current_step++);
		if (srh_mvs_cross_check(ctx_, slots.data(), nv, v, &params_) != SRH_OK) { error_ = srh_last_error(); checked = false; break; }
		if (isCancelled()) break;
	}
	if (speckleMinSize_ > 0 && checked && !isCancelled()) {
		// the speckle filter (not in the reference), every view in order, before anything reads the maps; the cross-check's
		// reject value (no step of its own: the step count is the reference's)
		srh_speckle_params s;
		srh_speckle_params_defaults(&s);
		s.min_size = speckleMinSize_; s.max_diff = speckleMaxDiff_; s.flags = SRH_SPECKLE_TO_NAN;
		for (int v = 0; v < nv; ++v) {
			const int rc = srh_view_filter_speckles(ctx_, v, &params_, &s, nullptr, nullptr);
			if (rc != SRH_OK && rc != SRH_E_CANCELLED) error_ = srh_last_error();
			if (rc != SRH_OK || isCancelled()) break;
		}
	}
	emitStage("Constructing depth maps");
	for (int v = 0; v < nv; ++v) {
		srh_view_depth_download(ctx_, v, computedDepths[v].data());
		colorize(v);
	}
	srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
}

srh_mvs_subpixel_info MultiViewStereo::subpixelInfo(CameraPtr view) const {
	for (size_t v = 0; v < views.size() && v < subpixelInfos_.size(); ++v)
		if (views[v] == view) return subpixelInfos_[v];
	return srh_mvs_subpixel_info();
}

srh_sgm_info MultiViewStereo::sgmInfo(CameraPtr view) const {
	for (size_t v = 0; v < views.size() && v < sgmInfos_.size(); ++v)
		if (views[v] == view) return sgmInfos_[v];
	return srh_sgm_info();
}

Image MultiViewStereo::depthMap(CameraPtr view) const {
	for (size_t v = 0; v < views.size(); ++v)
		if (views[v] == view) return results[v];
	return Image();                                    // unknown view => null image (:285)
}

const MultiViewStereo::DepthMap *MultiViewStereo::depths(CameraPtr view) const {
	for (size_t v = 0; v < views.size(); ++v)
		if (views[v] == view) return &computedDepths[v];
	return nullptr;
}

std::vector<PLYPoint> MultiViewStereo::pointCloud(CameraPtr view) {
	std::vector<PLYPoint> pts;
	for (size_t v = 0; v < views.size(); ++v) if (views[v] == view && ctx_) {
		const size_t n = static_cast<size_t>(images[v].w)*images[v].h;
		std::vector<double> xyz(3*n);
		std::vector<uint8_t> rgb(3*n), valid(n);
		params_.image_scale = imageScale;
		if (srh_view_depth_upload(ctx_, static_cast<int>(v), computedDepths[v].data()) != SRH_OK ||
		    srh_view_point_cloud(ctx_, static_cast<int>(v), &params_, xyz.data(), rgb.data(), valid.data(), nullptr, nullptr, nullptr) != SRH_OK) {
			error_ = srh_last_error();
			return pts;
		}
		for (size_t i = 0; i < n; ++i) if (valid[i]) {
			PLYPoint q;
			for (int k = 0; k < 3; ++k) { q.p[k] = xyz[3*i + k]; q.rgb[k] = rgb[3*i + k]; }
			pts.push_back(q);
		}
	}
	return pts;
}

std::vector<FusedPoint> MultiViewStereo::fusedPointCloud() {
	std::vector<FusedPoint> pts;
	const int nv = static_cast<int>(views.size());
	if (!ctx_ || nv == 0) return pts;
	params_.min_depth = minDepth; params_.max_depth = maxDepth; params_.num_depth_levels = numDepthLevels;
	params_.image_scale = imageScale; params_.cross_check_threshold = crossCheckThreshold;
	std::vector<int32_t> slots(nv);
	for (int v = 0; v < nv; ++v) {
		slots[v] = v;
		if (srh_view_depth_upload(ctx_, v, computedDepths[v].data()) != SRH_OK) { error_ = srh_last_error(); return pts; }
	}
	int64_t n = 0;
	if (srh_mvs_fuse(ctx_, slots.data(), nv, &params_, &fuseParams_, nullptr) != SRH_OK ||
	    srh_mvs_fused_count(ctx_, &n) != SRH_OK) { error_ = srh_last_error(); return pts; }
	const size_t k = static_cast<size_t>(n);
	std::vector<double> xyz(3*k), nrm(3*k);
	std::vector<uint8_t> rgb(3*k), nviews(k), flags(k);
	std::vector<int32_t> src(2*k);
	if (srh_mvs_fused_download(ctx_, 0, n, xyz.data(), nrm.data(), rgb.data(), nviews.data(), flags.data(), src.data()) != SRH_OK) {
		error_ = srh_last_error();
		return pts;
	}
	pts.resize(k);
	for (size_t i = 0; i < k; ++i) {
		FusedPoint &q = pts[i];
		for (int c = 0; c < 3; ++c) { q.p[c] = xyz[3*i + c]; q.n[c] = nrm[3*i + c]; q.rgb[c] = rgb[3*i + c]; }
		q.nviews = nviews[i]; q.flags = flags[i];
		q.view = src[2*i]; q.pixel = src[2*i + 1];
	}
	return pts;
}

double MultiViewStereo::coverage(CameraPtr view) const {
	for (size_t v = 0; v < views.size(); ++v) if (views[v] == view) {
		long total = 0, have = 0;
		for (size_t i = 0; i < masks[v].size(); ++i) if (masks[v][i] == 1) { ++total; if (std::isfinite(computedDepths[v][i])) ++have; }
		return total ? (100.0*have)/total : 0.0;
	}
	return 0.0;
}
