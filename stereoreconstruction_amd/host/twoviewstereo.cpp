// twoviewstereo.cpp -- host side of TwoViewStereo above the C-ABI (reference:
// stereo/twoviewstereo.cpp:89-227).  No arithmetic of the matching path happens here.
#include "twoviewstereo.hpp"

#include <cmath>
#include <limits>

namespace {
	void onProgress(int step, const char *stage, void *user);
}

struct TwoViewHooks {
	TwoViewStereo *self;
	std::function<void(int)> *progress;
	std::function<void(const std::string &)> *stage;
};

namespace {
	void onProgress(int step, const char *stage, void *user) {
		TwoViewHooks *h = static_cast<TwoViewHooks *>(user);
		if (*h->progress) (*h->progress)(step);
		if (*h->stage) (*h->stage)(stage);
	}
}

TwoViewStereo::TwoViewStereo(CameraPtr leftView_, Image left_, Image leftMask_,
                             CameraPtr rightView_, Image right_, Image rightMask_,
                             double minDepth_, double maxDepth_, int numDepthLevels_,
                             double imageScale_, int deviceOrdinal)
	: leftView(leftView_), rightView(rightView_)
	, left(left_), right(right_)
	, minDepth(minDepth_), maxDepth(maxDepth_), numDepthLevels(numDepthLevels_), imageScale(imageScale_)
	, ctx_(nullptr)
{
	// masks: null => all WHITE (twoviewstereo.cpp:105-113)
	leftMask = whiteMask(leftMask_, left.w, left.h);
	rightMask = whiteMask(rightMask_, right.w, right.h);
	setUp(deviceOrdinal);
}

// result images, depth maps and parameters for the images in hand; the context, unless the caller made it already
void TwoViewStereo::setUp(int deviceOrdinal) {
	resultLeft = Image(left.w, left.h);
	resultRight = Image(right.w, right.h);
	const double NaN = std::numeric_limits<double>::quiet_NaN();
	computedDepthLeft.assign(static_cast<size_t>(left.w)*left.h, NaN);
	computedDepthRight.assign(static_cast<size_t>(left.w)*left.h, NaN);   // sized from the LEFT image, as :119
	srh_params_twoview_defaults(&params_);
	params_.min_depth = minDepth; params_.max_depth = maxDepth;
	params_.num_depth_levels = numDepthLevels; params_.image_scale = imageScale;
	srh_twoview_mrf_params_defaults(&mrfParams_);
	mrfInfo_[0] = mrfInfo_[1] = srh_mrf_info();
	srh_twoview_sgm_params_defaults(&sgmParams_);
	sgmInfo_[0] = sgmInfo_[1] = srh_sgm_info();
	srh_rectify_params_defaults(&rectParams_);
	rectInfo_ = srh_rectify_info();
	rectCam_[0] = rectCam_[1] = srh_camera();
	if (!ctx_ && error_.empty() && srh_create(deviceOrdinal, &ctx_) != SRH_OK) { error_ = srh_last_error(); ctx_ = nullptr; }
}

TwoViewStereo::TwoViewStereo(ScaleOnDevice, CameraPtr leftView_, const Image &left_, const Image &leftMask_,
                             CameraPtr rightView_, const Image &right_, const Image &rightMask_,
                             double minDepth_, double maxDepth_, int numDepthLevels_,
                             double imageScale_, int deviceOrdinal)
	: leftView(leftView_), rightView(rightView_)
	, minDepth(minDepth_), maxDepth(maxDepth_), numDepthLevels(numDepthLevels_), imageScale(imageScale_)
	, ctx_(nullptr)
{
	// twoviewstereo.cpp:89-113: scaledToWidth(width*imageScale, Qt::SmoothTransformation) of both images and both masks
	if (srh_create(deviceOrdinal, &ctx_) != SRH_OK) { error_ = srh_last_error(); ctx_ = nullptr; }
	const Image *src[2] = { &left_, &right_ }, *msk[2] = { &leftMask_, &rightMask_ };
	Image *dst[2] = { &left, &right };
	std::vector<uint8_t> *dmask[2] = { &leftMask, &rightMask };
	CameraPtr cams[2] = { leftView, rightView };
	for (int s = 0; s < 2 && ctx_ && error_.empty(); ++s) {
		if (!cams[s] || src[s]->isNull()) { error_ = "null view or image"; break; }
		const srh_camera cam = cams[s]->snapshot();
		const bool hasMask = !msk[s]->isNull();
		int w = 0, h = 0;
		if (srh_view_upload_scaled(ctx_, s, src[s]->w, src[s]->h, src[s]->rgba.data(), src[s]->hasAlpha ? 1 : 0,
		                           hasMask ? msk[s]->rgba.data() : nullptr, msk[s]->w, msk[s]->h, msk[s]->hasAlpha ? 1 : 0,
		                           imageScale, SRH_MASK_IMAGE_SMOOTH, &cam) != SRH_OK ||
		    srh_view_size(ctx_, s, &w, &h) != SRH_OK) { error_ = srh_last_error(); break; }
		*dst[s] = Image(w, h);
		dst[s]->hasAlpha = src[s]->hasAlpha;
		dmask[s]->resize(static_cast<size_t>(w)*h);
		if (srh_view_image_download(ctx_, s, dst[s]->rgba.data(), dmask[s]->data()) != SRH_OK) { error_ = srh_last_error(); break; }
	}
	if (!error_.empty()) { left = right = Image(); leftMask.clear(); rightMask.clear(); }
	setUp(deviceOrdinal);
}

TwoViewStereo::~TwoViewStereo() { if (ctx_) srh_destroy(ctx_); }

void TwoViewStereo::colorFromDepth(double depth, uint8_t rgb[3]) const {
	// twoviewstereo.cpp:128-146 (QColor::fromHsvF(2t/3, 1, 1) restated; outside the numeric contract)
	rgb[0] = rgb[1] = rgb[2] = 0;
	if (std::isnan(depth) || std::isinf(depth)) return;
	const double t = (depth - minDepth) / (maxDepth - minDepth);
	if (t < 1e-5) return;
	if (t > 1.1) { rgb[0] = rgb[1] = rgb[2] = 255; return; }
	double h6 = (2.0*t/3.0)*6.0;
	h6 -= 6.0*std::floor(h6/6.0);
	const int sector = static_cast<int>(h6);
	const double f = h6 - sector, q = 1.0 - f;
	double r = 0, g = 0, b = 0;
	switch (sector) {
	case 0: r = 1; g = f; b = 0; break;
	case 1: r = q; g = 1; b = 0; break;
	case 2: r = 0; g = 1; b = f; break;
	case 3: r = 0; g = q; b = 1; break;
	case 4: r = f; g = 0; b = 1; break;
	default: r = 1; g = 0; b = q; break;
	}
	rgb[0] = static_cast<uint8_t>(std::lround(r*255)); rgb[1] = static_cast<uint8_t>(std::lround(g*255));
	rgb[2] = static_cast<uint8_t>(std::lround(b*255));
}

void TwoViewStereo::colorize(const DepthMap &d, Image &out) const {
	for (int y = 0; y < out.h; ++y)
		for (int x = 0; x < out.w; ++x) {
			uint8_t *p = out.pixel(x, y);
			colorFromDepth(d[static_cast<size_t>(y)*out.w + x], p);
			p[3] = 255;
		}
}

bool TwoViewStereo::uploadViews() {
	params_.min_depth = minDepth; params_.max_depth = maxDepth;
	params_.num_depth_levels = numDepthLevels; params_.image_scale = imageScale;
	const srh_camera lc = leftView->snapshot(), rc = rightView->snapshot();   // snapshot: the GUI may mutate cameras
	if (srh_view_upload(ctx_, 0, left.w, left.h, left.rgba.data(), leftMask.data(), &lc) != SRH_OK ||
	    srh_view_upload(ctx_, 1, right.w, right.h, right.rgba.data(), rightMask.data(), &rc) != SRH_OK) {
		error_ = srh_last_error();
		return false;
	}
	return true;
}

std::vector<std::pair<int, int> > TwoViewStereo::epipolarCurve(int x, int y, bool fromLeft) {
	std::vector<std::pair<int, int> > curve;
	if (!ctx_ || !leftView || !rightView || left.isNull() || right.isNull() || !uploadViews()) return curve;
	const int32_t xy[2] = { x, y };
	int32_t n = 0;
	std::vector<int32_t> pts(2*64);
	for (int attempt = 0; attempt < 2; ++attempt) {
		const int cap = static_cast<int>(pts.size()/2);
		if (srh_epipolar_curves(ctx_, fromLeft ? 0 : 1, fromLeft ? 1 : 0, &params_, 0, 1, xy, pts.data(), cap, &n) != SRH_OK) {
			error_ = srh_last_error();
			return curve;
		}
		if (n <= cap) break;
		pts.resize(2*static_cast<size_t>(n));
	}
	for (int i = 0; i < n; ++i) curve.push_back(std::make_pair(pts[2*i], pts[2*i + 1]));
	return curve;
}

double TwoViewStereo::pairCost(int kind, int x1, int y1, int x2, int y2, bool fromLeft) {
	double out = std::numeric_limits<double>::quiet_NaN();
	if (!ctx_ || !leftView || !rightView || left.isNull() || right.isNull() || !uploadViews()) return out;
	const int32_t xy[4] = { x1, y1, x2, y2 };
	if (srh_twoview_pair_costs(ctx_, fromLeft ? 0 : 1, fromLeft ? 1 : 0, &params_, kind, 1, xy, &out) != SRH_OK) {
		error_ = srh_last_error();
		return std::numeric_limits<double>::quiet_NaN();
	}
	return out;
}

double TwoViewStereo::cost_sad(int x1, int y1, int x2, int y2, bool fromLeft) {
	return pairCost(SRH_COST_SAD, x1, y1, x2, y2, fromLeft);
}

double TwoViewStereo::cost_census(int x1, int y1, int x2, int y2, bool fromLeft) {
	return pairCost(SRH_COST_CENSUS, x1, y1, x2, y2, fromLeft);
}

double TwoViewStereo::cost_ncc(int x1, int y1, int x2, int y2, bool fromLeft) {
	return pairCost(SRH_COST_NCC, x1, y1, x2, y2, fromLeft);
}

void TwoViewStereo::computeCostVolumes(CameraPtr leftView_, CameraPtr rightView_) {
	if (!ctx_ || !leftView_ || !rightView_) return;
	leftView = leftView_; rightView = rightView_;
	if (!uploadViews()) return;
	if (srh_set_option(ctx_, "cost", costKind) != SRH_OK) { error_ = srh_last_error(); return; }
	srh_set_option(ctx_, "sad_dense", sadDenseOn);
	srh_set_option(ctx_, "census_dense", censusDenseOn);
	if (srh_set_option(ctx_, "wta_outputs", wtaFlags) != SRH_OK) { error_ = srh_last_error(); return; }
	srh_set_option(ctx_, "subpixel", subpixelOn ? 1 : 0);
	if (srh_twoview_wta(ctx_, 0, 1, &params_, 0, 0) != SRH_OK || srh_twoview_wta(ctx_, 1, 0, &params_, 0, 0) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK) {
		error_ = srh_last_error();
		return;
	}
	fetchWtaOutputs();
}

// the kept by-products of both passes (leftSlot: the left map's, rightSlot: the right map's -- 0 and 1, or the rectified
// views' slots); empty when nothing was kept
void TwoViewStereo::fetchWtaOutputs(int leftSlot, int rightSlot) {
	for (int k = 0; k < 2; ++k) { winners_[k].clear(); runners_[k].clear(); minCosts_[k].clear(); secondCosts_[k].clear(); subDelta_[k].clear(); }
	if (!ctx_) return;
	// setSubpixel: the deltas of both passes (a slot whose map no scan made holds none: the vector stays empty)
	for (int k = 0; subpixelOn && k < 2; ++k) {
		const int slot = k == 0 ? leftSlot : rightSlot;
		int w = 0, h = 0;
		if (srh_view_size(ctx_, slot, &w, &h) != SRH_OK) { error_ = srh_last_error(); return; }
		subDelta_[k].resize(static_cast<size_t>(w)*h);
		if (srh_view_subpixel(ctx_, slot, subDelta_[k].data(), nullptr, nullptr) != SRH_OK) subDelta_[k].clear();
	}
	if (!wtaFlags) return;
	for (int k = 0; k < 2; ++k) {
		const int slot = k == 0 ? leftSlot : rightSlot;
		int flags = 0, w = 0, h = 0;
		if (srh_view_wta_outputs_state(ctx_, slot, &flags, nullptr) != SRH_OK || srh_view_size(ctx_, slot, &w, &h) != SRH_OK) { error_ = srh_last_error(); return; }
		if (!(flags & SRH_WTA_WINNERS)) continue;
		const size_t n = static_cast<size_t>(w)*h;
		const bool costs = (flags & SRH_WTA_COSTS) != 0;
		winners_[k].resize(2*n); runners_[k].resize(2*n);
		if (costs) { minCosts_[k].resize(n); secondCosts_[k].resize(n); }
		if (srh_view_wta_outputs(ctx_, slot, winners_[k].data(), runners_[k].data(), costs ? minCosts_[k].data() : nullptr,
		                         costs ? secondCosts_[k].data() : nullptr) != SRH_OK) {
			error_ = srh_last_error();
			winners_[k].clear(); runners_[k].clear(); minCosts_[k].clear(); secondCosts_[k].clear();
			return;
		}
	}
}

void TwoViewStereo::crossCheck(CameraPtr leftView_, CameraPtr rightView_) {
	if (!ctx_ || !leftView_ || !rightView_) return;
	leftView = leftView_; rightView = rightView_;
	if (!uploadViews()) return;
	if (srh_view_depth_upload(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_upload(ctx_, 1, computedDepthRight.data()) != SRH_OK ||
	    srh_twoview_cross_check(ctx_, 0, 1, &params_) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK)
		error_ = srh_last_error();
}

void TwoViewStereo::filterInvalidPixels() {
	if (!ctx_) return;
	const int flags = filterFlags ? filterFlags : SRH_FILTER_GAPS;
	TwoViewHooks hooks = { this, &progressUpdate, &stageUpdate };
	srh_set_hooks(ctx_, cancelFlag(), onProgress, &hooks);
	emitProgress(6);
	emitStage("Filling invalid pixels...");
	if (flags & SRH_FILTER_MEDIAN) { emitProgress(7); emitStage("Filtering invalid pixels..."); }
	int rc = srh_view_depth_upload(ctx_, 0, computedDepthLeft.data());
	if (rc == SRH_OK) rc = srh_view_depth_upload(ctx_, 1, computedDepthRight.data());
	// (the reference's right-map loop tests left.width() (:748): the views are equal-sized, each map is filled over its own)
	if (rc == SRH_OK) rc = srh_view_filter_invalid(ctx_, 0, &params_, flags, 2, nullptr);
	if (rc == SRH_OK && !isCancelled()) rc = srh_view_filter_invalid(ctx_, 1, &params_, flags, 2, nullptr);
	if (rc == SRH_OK) rc = srh_view_depth_download(ctx_, 0, computedDepthLeft.data());
	if (rc == SRH_OK) rc = srh_view_depth_download(ctx_, 1, computedDepthRight.data());
	srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
	if (rc != SRH_OK && rc != SRH_E_CANCELLED) error_ = srh_last_error();
}

void TwoViewStereo::filterSpeckles() {
	if (!ctx_ || speckleMinSize <= 0) return;
	if (speckleDiffSteps < 1) { error_ = "speckle filter: diffSteps must be >= 1"; return; }
	srh_speckle_params s;
	srh_speckle_params_defaults(&s);
	s.min_size = speckleMinSize;
	s.max_diff = static_cast<double>(speckleDiffSteps) * ((params_.max_depth - params_.min_depth)/static_cast<double>(params_.num_depth_levels - 1));
	TwoViewHooks hooks = { this, &progressUpdate, &stageUpdate };
	srh_set_hooks(ctx_, cancelFlag(), onProgress, &hooks);
	emitProgress(5);
	emitStage("Removing speckles...");
	int rc = srh_view_depth_upload(ctx_, 0, computedDepthLeft.data());
	if (rc == SRH_OK) rc = srh_view_depth_upload(ctx_, 1, computedDepthRight.data());
	if (rc == SRH_OK) rc = srh_view_filter_speckles(ctx_, 0, &params_, &s, nullptr, nullptr);
	if (rc == SRH_OK && !isCancelled()) rc = srh_view_filter_speckles(ctx_, 1, &params_, &s, nullptr, nullptr);
	if (rc == SRH_OK) rc = srh_view_depth_download(ctx_, 0, computedDepthLeft.data());
	if (rc == SRH_OK) rc = srh_view_depth_download(ctx_, 1, computedDepthRight.data());
	srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
	if (rc != SRH_OK && rc != SRH_E_CANCELLED) error_ = srh_last_error();
}

double TwoViewStereo::depthFromLabel(int label) const {
	double t = static_cast<double>(label) / (numDepthLevels - 1);
	t /= (5.0 - 4.0*t);
	return minDepth*(1.0 - t) + maxDepth*t;
}

// setRectify(true): slots 0, 1 (uploaded) warped into slots 2, 3, and the rectified products of the views kept.  false: the
// library refused the pair (lastError() says why) -- nothing is rectified and the rectified products are empty.
bool TwoViewStereo::rectifyViews() {
	rectInfo_ = srh_rectify_info();
	for (int k = 0; k < 2; ++k) { rectDepth_[k].clear(); rectImage_[k] = Image(); rectMask_[k].clear(); rectCam_[k] = srh_camera(); }
	const srh_camera lc = leftView->snapshot(), rc = rightView->snapshot();
	if (srh_rectify_cameras(&lc, &rc, left.w, left.h, params_.image_scale, &rectParams_, &rectCam_[0], &rectCam_[1]) != SRH_OK ||
	    srh_twoview_rectify(ctx_, 0, 1, 2, 3, &params_, &rectParams_, &rectInfo_) != SRH_OK) {
		error_ = srh_last_error();
		rectCam_[0] = rectCam_[1] = srh_camera();
		return false;
	}
	for (int k = 0; k < 2; ++k) {
		int w = 0, h = 0;
		if (srh_view_size(ctx_, 2 + k, &w, &h) != SRH_OK) { error_ = srh_last_error(); return false; }
		rectImage_[k] = Image(w, h);
		rectMask_[k].resize(static_cast<size_t>(w)*h);
		rectDepth_[k].assign(static_cast<size_t>(w)*h, std::numeric_limits<double>::quiet_NaN());
		if (srh_view_image_download(ctx_, 2 + k, rectImage_[k].rgba.data(), rectMask_[k].data()) != SRH_OK) { error_ = srh_last_error(); return false; }
	}
	return true;
}

// the rectified maps (slots 2, 3, as the pipeline left them) into the views the caller handed in (slots 0, 1)
bool TwoViewStereo::unrectifyMaps() {
	if (srh_view_depth_unrectify(ctx_, 2, 0, &params_, nullptr) != SRH_OK || srh_view_depth_unrectify(ctx_, 3, 1, &params_, nullptr) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK) {
		error_ = srh_last_error();
		return false;
	}
	return true;
}

void TwoViewStereo::computeDepthMaps() {
	// twoviewstereo.cpp:150-227: cost volumes (steps 1,3; setUseMRF / setUseSGM: + the optimiser / the aggregation, 2,4), cross-check (5), colourise, finished (8)
	if (!ctx_) { if (error_.empty()) error_ = "no device context"; return; }
	if (!leftView || !rightView || left.isNull() || right.isNull()) { error_ = "missing view"; return; }
	if (!uploadViews()) return;
	TwoViewHooks hooks = { this, &progressUpdate, &stageUpdate };
	srh_set_hooks(ctx_, cancelFlag(), onProgress, &hooks);
	srh_set_option(ctx_, "filter_invalid", filterFlags);
	srh_set_option(ctx_, "sad_dense", sadDenseOn);
	srh_set_option(ctx_, "census_dense", censusDenseOn);
	srh_set_option(ctx_, "subpixel", subpixelOn ? 1 : 0);
	if (srh_set_option(ctx_, "speckle_min_size", speckleMinSize) != SRH_OK ||
	    (speckleMinSize && srh_set_option(ctx_, "speckle_diff_steps", speckleDiffSteps) != SRH_OK) ||
	    srh_set_option(ctx_, "cost", costKind) != SRH_OK || srh_set_option(ctx_, "wta_outputs", wtaFlags) != SRH_OK) {
		error_ = srh_last_error();
		srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
		return;
	}
	mrfInfo_[0] = mrfInfo_[1] = srh_mrf_info();
	sgmInfo_[0] = sgmInfo_[1] = srh_sgm_info();
	// setRectify: the pipeline runs on the rectified views (slots 2, 3) into the rectified maps; a refused pair runs as it is
	rectified_ = rectifyOn && rectifyViews();
	const int ls = rectified_ ? 2 : 0, rs = rectified_ ? 3 : 1;
	double *dl = rectified_ ? rectDepth_[0].data() : computedDepthLeft.data(), *dr = rectified_ ? rectDepth_[1].data() : computedDepthRight.data();
	const int rc_ = useSgm ? srh_twoview_compute_sgm(ctx_, ls, rs, &params_, &sgmParams_, dl, dr, sgmInfo_)
	              : useMrf ? srh_twoview_compute_mrf(ctx_, ls, rs, &params_, &mrfParams_, dl, dr, mrfInfo_)
	                       : srh_twoview_compute(ctx_, ls, rs, &params_, dl, dr);
	srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
	if (rc_ == SRH_E_CANCELLED) return;              // reference: silent return on cancel
	if (rc_ != SRH_OK) { error_ = srh_last_error(); return; }
	fetchWtaOutputs(ls, rs);
	if (rectified_ && !unrectifyMaps()) return;
	colorize(computedDepthLeft, resultLeft);
	colorize(computedDepthRight, resultRight);
}
