// stereo_qt.cpp -- see stereo_qt.hpp.  No arithmetic of the matching path happens here: images are decoded and
// scaled by Qt exactly where the reference does it, everything else is the C-ABI.
#include "stereo_qt.hpp"

#include <QtCore/QFileInfo>
#include <QtGui/QColor>

#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>

namespace srq {

Raster rasterFromQImage(const QImage &in) {
	Raster r;
	if (in.isNull()) return r;
	const QImage img = in.depth() == 32 ? in : in.convertToFormat(QImage::Format_ARGB32);
	r.w = img.width(); r.h = img.height();
	r.rgba.resize(static_cast<size_t>(r.w)*r.h*4);
	for (int y = 0; y < r.h; ++y) {
		const QRgb *scanline = reinterpret_cast<const QRgb *>(img.constScanLine(y));
		unsigned char *out = &r.rgba[static_cast<size_t>(y)*r.w*4];
		for (int x = 0; x < r.w; ++x, out += 4) {
			const QRgb rgb = scanline[x];
			out[0] = static_cast<unsigned char>(qRed(rgb)); out[1] = static_cast<unsigned char>(qGreen(rgb));
			out[2] = static_cast<unsigned char>(qBlue(rgb)); out[3] = static_cast<unsigned char>(qAlpha(rgb));
		}
	}
	return r;
}

void writePLY(const std::string &path, size_t npoints, const double *xyz, const unsigned char *rgb) {
	std::ofstream lout(path.c_str());
	lout << "ply\n" << "format ascii 1.0\n" << "element vertex " << npoints << "\n"
	     << "property float x\n" << "property float y\n" << "property float z\n"
	     << "property uchar diffuse_red\n" << "property uchar diffuse_green\n" << "property uchar diffuse_blue\n"
	     << "end_header\n";
	for (size_t i = 0; i < npoints; ++i)
		lout << xyz[i*3] << ' ' << xyz[i*3 + 1] << ' ' << xyz[i*3 + 2] << ' ' << static_cast<int>(rgb[i*3]) << ' '
		     << static_cast<int>(rgb[i*3 + 1]) << ' ' << static_cast<int>(rgb[i*3 + 2]) << '\n';
}

void writePLY(const std::string &path, size_t npoints, const double *xyz, const int *rgb) {
	std::ofstream lout(path.c_str());
	lout << "ply\n" << "format ascii 1.0\n" << "element vertex " << npoints << "\n"
	     << "property float x\n" << "property float y\n" << "property float z\n"
	     << "property uchar diffuse_red\n" << "property uchar diffuse_green\n" << "property uchar diffuse_blue\n"
	     << "end_header\n";
	for (size_t i = 0; i < npoints; ++i)
		lout << xyz[i*3] << ' ' << xyz[i*3 + 1] << ' ' << xyz[i*3 + 2] << ' ' << rgb[i*3] << ' ' << rgb[i*3 + 1] << ' ' << rgb[i*3 + 2] << '\n';
}

} // namespace srq

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

namespace srq {

std::vector<unsigned char> whiteMask(const Raster &m) {
	std::vector<unsigned char> out(static_cast<size_t>(m.w)*m.h);
	for (size_t i = 0; i < out.size(); ++i) {
		const unsigned char *p = &m.rgba[i*4];
		out[i] = (p[0] == 255 && p[1] == 255 && p[2] == 255 && p[3] == 255) ? 1 : 0;
	}
	return out;
}

bool ingestViewFile(const QString &file, double imageScale, Raster &image, std::vector<unsigned char> &mask) {
	if (!QFileInfo(file).exists()) return false;
	QImage baseImage(file);
	if (baseImage.isNull()) return false;
	const QImage scaled = baseImage.scaledToWidth(static_cast<int>(baseImage.width() * imageScale), Qt::SmoothTransformation);
	image = rasterFromQImage(scaled);
	mask.assign(static_cast<size_t>(image.w)*image.h, 1);
	if (baseImage.hasAlphaChannel()) {
		const QImage m = baseImage.scaledToWidth(scaled.width(), Qt::FastTransformation);
		for (int y = 0; y < m.height() && y < image.h; ++y)
			for (int x = 0; x < m.width() && x < image.w; ++x)
				if (qAlpha(m.pixel(x, y)) != 255) mask[static_cast<size_t>(y)*image.w + x] = 0;   // not fully opaque: ignored
	}
	return true;
}

} // namespace srq

// ------------------------------------------------------------------ TwoViewStereo
static int g_device = 0;
void TwoViewStereo::setDevice(int ordinal) { g_device = ordinal; }
void MultiViewStereo::setDevice(int ordinal) { g_device = ordinal; }

TwoViewStereo::TwoViewStereo(CameraPtr leftView_, QImage left_, QImage leftMask_,
                             CameraPtr rightView_, QImage right_, QImage rightMask_,
                             double minDepth_, double maxDepth_, int numDepthLevels_, double imageScale_)
	: leftView(leftView_), rightView(rightView_)
	, minDepth(minDepth_), maxDepth(maxDepth_), numDepthLevels(numDepthLevels_), imageScale(imageScale_), ctx_(nullptr)
{
	const int deviceOrdinal = g_device;
	memset(&leftCam, 0, sizeof(leftCam)); memset(&rightCam, 0, sizeof(rightCam));
	if (leftView) leftCam = srq::cameraInfo(*leftView).camera;         // the host application's glue (stereo_qt.hpp)
	if (rightView) rightCam = srq::cameraInfo(*rightView).camera;
	// twoviewstereo.cpp:89-124: images and masks are smooth-scaled to width*imageScale; a null mask is all WHITE
	left = srq::rasterFromQImage(left_.scaledToWidth(static_cast<int>(left_.width() * imageScale), Qt::SmoothTransformation));
	right = srq::rasterFromQImage(right_.scaledToWidth(static_cast<int>(right_.width() * imageScale), Qt::SmoothTransformation));
	if (!leftMask_.isNull())
		leftMask = srq::whiteMask(srq::rasterFromQImage(leftMask_.scaledToWidth(static_cast<int>(leftMask_.width() * imageScale), Qt::SmoothTransformation)));
	else leftMask.assign(static_cast<size_t>(left.w)*left.h, 1);
	if (!rightMask_.isNull())
		rightMask = srq::whiteMask(srq::rasterFromQImage(rightMask_.scaledToWidth(static_cast<int>(rightMask_.width() * imageScale), Qt::SmoothTransformation)));
	else rightMask.assign(static_cast<size_t>(right.w)*right.h, 1);
	const double NaN = std::numeric_limits<double>::quiet_NaN();
	computedDepthLeft.assign(static_cast<size_t>(left.w)*left.h, NaN);
	computedDepthRight.assign(static_cast<size_t>(left.w)*left.h, NaN);      // sized from the LEFT image, as :119
	srh_params_twoview_defaults(&params_);
	srh_twoview_mrf_params_defaults(&mrfParams_);
	mrfInfo_[0] = mrfInfo_[1] = srh_mrf_info();
	srh_twoview_sgm_params_defaults(&sgmParams_);
	sgmInfo_[0] = sgmInfo_[1] = srh_sgm_info();
	srh_rectify_params_defaults(&rectParams_);
	rectInfo_ = srh_rectify_info();
	rectCam_[0] = rectCam_[1] = srh_camera();
	if (srh_create(deviceOrdinal, &ctx_) != SRH_OK) { error_ = srh_last_error(); ctx_ = nullptr; }
}

namespace { void relayToTwoView(int step, const char *stage, void *user) { static_cast<TwoViewStereo *>(user)->relayProgress(step, stage); } }

void TwoViewStereo::relayProgress(int step, const char *stage) {
	if (isCancelled()) cancelWord_ = 1;
	emit progressUpdate(step);
	emit stageUpdate(QString::fromLatin1(stage));
}

TwoViewStereo::~TwoViewStereo() { if (ctx_) srh_destroy(ctx_); }

QImage TwoViewStereo::colorize(const DepthMap &d, int w, int h) const {
	// twoviewstereo.cpp:128-146 + VectorImage::toQImage(.., false)
	QImage out(w, h, QImage::Format_ARGB32);
	for (int y = 0; y < h; ++y) {
		QRgb *scanline = reinterpret_cast<QRgb *>(out.scanLine(y));
		for (int x = 0; x < w; ++x) {
			const double depth = d[static_cast<size_t>(y)*w + x];
			QRgb px = qRgba(0, 0, 0, 255);
			if (!std::isnan(depth) && !std::isinf(depth)) {
				const double t = (depth - minDepth) / (maxDepth - minDepth);
				if (t > 1.1) px = qRgba(255, 255, 255, 255);
				else if (!(t < 1e-5)) { const QColor c = QColor::fromHsvF(2.0 * t / 3.0, 1.0, 1.0); px = qRgba(c.red(), c.green(), c.blue(), 255); }
			}
			scanline[x] = px;
		}
	}
	return out;
}

bool TwoViewStereo::uploadViews() const {
	if (uploaded_) return true;
	if (srh_view_upload(ctx_, 0, left.w, left.h, left.rgba.data(), leftMask.data(), &leftCam) != SRH_OK ||
	    srh_view_upload(ctx_, 1, right.w, right.h, right.rgba.data(), rightMask.data(), &rightCam) != SRH_OK) {
		error_ = srh_last_error(); return false;
	}
	uploaded_ = true;
	return true;
}

std::vector<std::array<double, 3> > TwoViewStereo::curveOfPixel(int x, int y, bool fromLeft) const {
	std::vector<std::array<double, 3> > curve;
	if (!ctx_ || left.w <= 0 || right.w <= 0 || !uploadViews()) return curve;
	srh_params p = params_;
	p.min_depth = minDepth; p.max_depth = maxDepth; p.num_depth_levels = numDepthLevels; p.image_scale = imageScale;
	const int32_t xy[2] = { x, y };
	int32_t count = 0;
	std::vector<int32_t> pts(2*256);
	for (int pass = 0; pass < 2; ++pass) {                  // the curve's length is only known afterwards
		if (srh_epipolar_curves(ctx_, fromLeft ? 0 : 1, fromLeft ? 1 : 0, &p, 0, 1, xy, pts.data(),
		                        static_cast<int>(pts.size()/2), &count) != SRH_OK) { error_ = srh_last_error(); return curve; }
		if (static_cast<size_t>(count) <= pts.size()/2) break;
		pts.resize(2*static_cast<size_t>(count));
	}
	curve.resize(static_cast<size_t>(count));
	for (int k = 0; k < count; ++k) curve[k] = { static_cast<double>(pts[2*k]), static_cast<double>(pts[2*k + 1]), 1.0 };
	return curve;
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

// setRectify(true): slots 0, 1 (uploaded) warped into slots 2, 3, and the rectified products of the views kept.  false: the
// library refused the pair (lastError() says why) -- nothing is rectified and the rectified products are empty.
bool TwoViewStereo::rectifyViews() {
	rectInfo_ = srh_rectify_info();
	for (int k = 0; k < 2; ++k) { rectDepth_[k].clear(); rectImage_[k] = QImage(); rectCam_[k] = srh_camera(); }
	if (srh_rectify_cameras(&leftCam, &rightCam, left.w, left.h, params_.image_scale, &rectParams_, &rectCam_[0], &rectCam_[1]) != SRH_OK ||
	    srh_twoview_rectify(ctx_, 0, 1, 2, 3, &params_, &rectParams_, &rectInfo_) != SRH_OK) {
		error_ = srh_last_error();
		rectCam_[0] = rectCam_[1] = srh_camera();
		return false;
	}
	for (int k = 0; k < 2; ++k) {
		int w = 0, h = 0;
		if (srh_view_size(ctx_, 2 + k, &w, &h) != SRH_OK) { error_ = srh_last_error(); return false; }
		std::vector<unsigned char> rgba(static_cast<size_t>(w)*h*4);
		if (srh_view_image_download(ctx_, 2 + k, rgba.data(), nullptr) != SRH_OK) { error_ = srh_last_error(); return false; }
		rectImage_[k] = QImage(rgba.data(), w, h, 4*w, QImage::Format_RGBA8888).copy();      // (deep copy: `rgba` goes away)
		rectDepth_[k].assign(static_cast<size_t>(w)*h, std::numeric_limits<double>::quiet_NaN());
	}
	return true;
}

void TwoViewStereo::computeDepthMaps() {
	// twoviewstereo.cpp:150-227: cost volumes (steps 1, 3), cross-check (5), colourise, finished (8).
	// Errors are silent, as in the reference; lastError() keeps the library's message.
	if (!ctx_ || left.w <= 0 || right.w <= 0) return;
	if (left.w != right.w || left.h != right.h) { error_ = "views differ in size"; return; }
	params_.min_depth = minDepth; params_.max_depth = maxDepth;
	params_.num_depth_levels = numDepthLevels; params_.image_scale = imageScale;
	if (!uploadViews()) return;
	if (srh_set_option(ctx_, "cost", costKind) != SRH_OK) { error_ = srh_last_error(); return; }
	srh_set_option(ctx_, "sad_dense", sadDenseOn);
	srh_set_option(ctx_, "census_dense", censusDenseOn);
	if (srh_set_option(ctx_, "wta_outputs", wtaFlags) != SRH_OK) { error_ = srh_last_error(); return; }
	srh_set_option(ctx_, "subpixel", subpixelOn ? 1 : 0);
	mrfInfo_[0] = mrfInfo_[1] = srh_mrf_info();
	sgmInfo_[0] = sgmInfo_[1] = srh_sgm_info();
	// setRectify: the pipeline runs on the rectified views (slots 2, 3) into the rectified maps; a refused pair runs as it is
	rectified_ = rectifyOn && rectifyViews();
	if (useMrf || useSgm || rectified_) {
		// a USE_MRF build, the semi-global aggregation, or a rectified pair: the library sequences the run and reports the
		// steps (1, 2, 3, 4, 5, [6, 7,] 8) through its hook
		const int ls = rectified_ ? 2 : 0, rs = rectified_ ? 3 : 1;
		double *dl = rectified_ ? rectDepth_[0].data() : computedDepthLeft.data(), *dr = rectified_ ? rectDepth_[1].data() : computedDepthRight.data();
		cancelWord_ = isCancelled() ? 1 : 0;
		srh_set_hooks(ctx_, &cancelWord_, relayToTwoView, this);
		srh_set_option(ctx_, "filter_invalid", filterFlags);
		if (srh_set_option(ctx_, "speckle_min_size", speckleMinSize) != SRH_OK ||
		    (speckleMinSize && srh_set_option(ctx_, "speckle_diff_steps", speckleDiffSteps) != SRH_OK)) {
			error_ = srh_last_error();
			srh_set_option(ctx_, "filter_invalid", 0);
			srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
			return;
		}
		const int rc = useSgm ? srh_twoview_compute_sgm(ctx_, ls, rs, &params_, &sgmParams_, dl, dr, sgmInfo_)
		             : useMrf ? srh_twoview_compute_mrf(ctx_, ls, rs, &params_, &mrfParams_, dl, dr, mrfInfo_)
		                      : srh_twoview_compute(ctx_, ls, rs, &params_, dl, dr);
		srh_set_option(ctx_, "filter_invalid", 0);
		srh_set_option(ctx_, "speckle_min_size", 0);
		srh_set_hooks(ctx_, nullptr, nullptr, nullptr);
		if (rc == SRH_E_CANCELLED) return;
		if (rc != SRH_OK) { error_ = srh_last_error(); return; }
		fetchWtaOutputs(ls, rs);                            // (MRF / SGM: no scan made these maps, the vectors come back empty)
		if (rectified_ &&                                   // the rectified maps into the views the caller handed in
		    (srh_view_depth_unrectify(ctx_, 2, 0, &params_, nullptr) != SRH_OK || srh_view_depth_unrectify(ctx_, 3, 1, &params_, nullptr) != SRH_OK ||
		     srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
		     srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK)) { error_ = srh_last_error(); return; }
		resultLeft = colorize(computedDepthLeft, left.w, left.h);
		resultRight = colorize(computedDepthRight, right.w, right.h);
		return;
	}
	emit progressUpdate(1);
	emit stageUpdate("Computing cost volume for left image...");
	if (srh_twoview_wta(ctx_, 0, 1, &params_, 0, 0) != SRH_OK) { error_ = srh_last_error(); return; }
	if (isCancelled()) return;
	emit progressUpdate(3);
	emit stageUpdate("Computing cost volume for right image...");
	if (srh_twoview_wta(ctx_, 1, 0, &params_, 0, 0) != SRH_OK) { error_ = srh_last_error(); return; }
	if (isCancelled()) return;
	emit progressUpdate(5);
	emit stageUpdate("Detecting inconsistencies...");
	if (srh_twoview_cross_check(ctx_, 0, 1, &params_) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK) { error_ = srh_last_error(); return; }
	if (isCancelled()) return;
	fetchWtaOutputs();
	if (!error_.isEmpty()) return;
	if (speckleMinSize > 0) {
		filterSpeckles();
		if (isCancelled() || !error_.isEmpty()) return;
	}
	if (filterFlags) {
		filterInvalidPixels();
		if (isCancelled() || !error_.isEmpty()) return;
	}
	resultLeft = colorize(computedDepthLeft, left.w, left.h);
	resultRight = colorize(computedDepthRight, right.w, right.h);
	emit progressUpdate(8);
	emit stageUpdate("Finished!");
}

double TwoViewStereo::pairCost(int kind, int x1, int y1, int x2, int y2, bool fromLeft) {
	double out = std::numeric_limits<double>::quiet_NaN();
	if (!ctx_ || left.w <= 0 || right.w <= 0 || !uploadViews()) return out;
	srh_params p = params_;
	p.min_depth = minDepth; p.max_depth = maxDepth; p.num_depth_levels = numDepthLevels; p.image_scale = imageScale;
	const int32_t xy[4] = { x1, y1, x2, y2 };
	if (srh_twoview_pair_costs(ctx_, fromLeft ? 0 : 1, fromLeft ? 1 : 0, &p, kind, 1, xy, &out) != SRH_OK) {
		error_ = srh_last_error();
		return std::numeric_limits<double>::quiet_NaN();
	}
	return out;
}

double TwoViewStereo::cost_sad(int x1, int y1, int x2, int y2, bool fromLeft) { return pairCost(SRH_COST_SAD, x1, y1, x2, y2, fromLeft); }
double TwoViewStereo::cost_census(int x1, int y1, int x2, int y2, bool fromLeft) { return pairCost(SRH_COST_CENSUS, x1, y1, x2, y2, fromLeft); }
double TwoViewStereo::cost_ncc(int x1, int y1, int x2, int y2, bool fromLeft) { return pairCost(SRH_COST_NCC, x1, y1, x2, y2, fromLeft); }

void TwoViewStereo::filterInvalidPixels() {
	if (!ctx_ || !uploadViews()) return;
	const int flags = filterFlags ? filterFlags : SRH_FILTER_GAPS;
	emit progressUpdate(6);
	emit stageUpdate("Filling invalid pixels...");
	if (srh_view_depth_upload(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_upload(ctx_, 1, computedDepthRight.data()) != SRH_OK) { error_ = srh_last_error(); return; }
	if (flags & SRH_FILTER_MEDIAN) {
		emit progressUpdate(7);
		emit stageUpdate("Filtering invalid pixels...");
	}
	if (isCancelled()) return;
	// (the reference's right-map loop tests left.width() (:748): the views are equal-sized, each map is filled over its own)
	if (srh_view_filter_invalid(ctx_, 0, &params_, flags, 2, nullptr) != SRH_OK ||
	    srh_view_filter_invalid(ctx_, 1, &params_, flags, 2, nullptr) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK) error_ = srh_last_error();
}

void TwoViewStereo::filterSpeckles() {
	if (!ctx_ || speckleMinSize <= 0 || !uploadViews()) return;
	if (speckleDiffSteps < 1) { error_ = "speckle filter: diffSteps must be >= 1"; return; }
	srh_speckle_params s;
	srh_speckle_params_defaults(&s);
	s.min_size = speckleMinSize;
	s.max_diff = static_cast<double>(speckleDiffSteps) * ((params_.max_depth - params_.min_depth)/static_cast<double>(params_.num_depth_levels - 1));
	emit progressUpdate(5);
	emit stageUpdate("Removing speckles...");
	if (srh_view_depth_upload(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_upload(ctx_, 1, computedDepthRight.data()) != SRH_OK ||
	    srh_view_filter_speckles(ctx_, 0, &params_, &s, nullptr, nullptr) != SRH_OK ||
	    srh_view_filter_speckles(ctx_, 1, &params_, &s, nullptr, nullptr) != SRH_OK ||
	    srh_view_depth_download(ctx_, 0, computedDepthLeft.data()) != SRH_OK ||
	    srh_view_depth_download(ctx_, 1, computedDepthRight.data()) != SRH_OK) error_ = srh_last_error();
}

// ------------------------------------------------------------------ MultiViewStereo
MultiViewStereo::MultiViewStereo()
	: minDepth(0), maxDepth(0), crossCheckThreshold(0), imageScale(1), numDepthLevels(0), ctx_(nullptr)
{
	const int deviceOrdinal = g_device;
	srh_params_mvs_defaults(&params_);
	srh_mrf_params_defaults(&mrfParams_);
	srh_mvs_sgm_params_defaults(&sgmParams_);
	srh_fuse_params_defaults(&fuseParams_);
	if (srh_create(deviceOrdinal, &ctx_) != SRH_OK) { error_ = srh_last_error(); ctx_ = nullptr; }
}

MultiViewStereo::~MultiViewStereo() { if (ctx_) srh_destroy(ctx_); }

void MultiViewStereo::initialize(ProjectPtr project_, ImageSetPtr imageSet, const std::vector<CameraPtr> &views,
                                 double minDepth_, double maxDepth_, int numDepthLevels_, double crossCheckThreshold_, double imageScale_)
{
	// multiviewstereo.cpp:193-247: every non-null view with a default image in the set becomes a record
	std::vector<View> records;
	for (size_t index = 0; index < views.size(); ++index) if (views[index] && imageSet) {
		const srq::CameraInfo info = srq::cameraInfo(*views[index]);
		View v;
		v.id = info.id; v.name = info.name; v.camera = info.camera; v.ptr = views[index];
		v.file = srq::defaultImageFile(*imageSet, views[index]);
		if (!v.file.isEmpty()) records.push_back(v);
	}
	initialize(records, minDepth_, maxDepth_, numDepthLevels_, crossCheckThreshold_, imageScale_);
	project = project_;
	imageSet_ = imageSet;
}

void MultiViewStereo::initialize(const std::vector<View> &views, double minDepth_, double maxDepth_, int numDepthLevels_,
                                 double crossCheckThreshold_, double imageScale_)
{
	project.reset(); imageSet_.reset();
	minDepth = minDepth_; maxDepth = maxDepth_; numDepthLevels = numDepthLevels_;
	crossCheckThreshold = crossCheckThreshold_; imageScale = imageScale_;
	views_.clear(); images.clear(); masks.clear(); results.clear(); computedDepths.clear();
	const double NaN = std::numeric_limits<double>::quiet_NaN();
	for (size_t i = 0; i < views.size() && views_.size() < static_cast<size_t>(SRH_MAX_VIEWS); ++i) {
		srq::Raster img; std::vector<unsigned char> m;
		if (!srq::ingestViewFile(views[i].file, imageScale, img, m)) continue;       // no file: the view is skipped (:214)
		images.push_back(img); masks.push_back(m);
		results.push_back(QImage());
		computedDepths.push_back(std::vector<double>(static_cast<size_t>(img.w)*img.h, NaN));
		views_.push_back(views[i]);
	}
}

void MultiViewStereo::colorize(int v) {
	// multiviewstereo.cpp:252-276, 382-395: black = close, white = far; NaN / INF / unknown (-1) and masked-out: white
	const int w = images[v].w, h = images[v].h;
	QImage out(w, h, QImage::Format_ARGB32);
	for (int y = 0; y < h; ++y) {
		QRgb *scanline = reinterpret_cast<QRgb *>(out.scanLine(y));
		for (int x = 0; x < w; ++x) {
			int gray = 255;
			if (masks[v][static_cast<size_t>(y)*w + x] == 1) {
				const double d = computedDepths[v][static_cast<size_t>(y)*w + x];
				if (!std::isnan(d) && !std::isinf(d) && !(d + 1e-5 < minDepth)) {
					const double t = std::min(1.0, std::max(0.0, (d - minDepth) / (maxDepth - minDepth)));
					gray = static_cast<int>(255*t);          // RGBA(255*t) stored as double, truncated by qRgba's int parameters
				}
			}
			scanline[x] = qRgba(gray, gray, gray, 255);
		}
	}
	results[v] = out;
}

void MultiViewStereo::runTask() {
	// multiviewstereo.cpp:325-475: neighbours, initial estimates (steps 0..V-1), colourise, cross-checks in view
	// order (steps V..2V-1), colourise.  Invalid state: silent return (:326-327).
	const int V = static_cast<int>(views_.size());
	if (!ctx_ || V == 0) return;
	params_.min_depth = minDepth; params_.max_depth = maxDepth; params_.num_depth_levels = numDepthLevels;
	params_.image_scale = imageScale; params_.cross_check_threshold = crossCheckThreshold;
	std::vector<srh_camera> cams(V);
	std::vector<int32_t> slotIds(V);
	for (int v = 0; v < V; ++v) {
		cams[v] = views_[v].camera; slotIds[v] = v;
		if (srh_view_upload(ctx_, v, images[v].w, images[v].h, images[v].rgba.data(), masks[v].data(), &cams[v]) != SRH_OK) {
			error_ = srh_last_error(); return;
		}
	}
	const int nn = params_.num_neighbours > 0 ? params_.num_neighbours : 1;
	std::vector<int32_t> neigh(static_cast<size_t>(V)*nn), count(V);
	if (srh_mvs_neighbours(V, cams.data(), &params_, neigh.data(), count.data()) != SRH_OK) { error_ = srh_last_error(); return; }
	int step = 0;
	for (int v = 0; v < V; ++v) {
		if (isCancelled()) return;
		emit progressUpdate(step++);
		emit stageUpdate(tr("Computing cost volume for camera %1").arg(views_[v].name));
		const int32_t *nb = &neigh[static_cast<size_t>(v)*nn];
		if ((useMrf_ || useSgm_ ? srh_mvs_initial_estimate_peaks(ctx_, v, nb, count[v], &params_)                        // #ifdef USE_MRF: peaks kept,
		             : srh_mvs_initial_estimate(ctx_, v, nb, count[v], &params_, 0, 0, nullptr)) != SRH_OK) { error_ = srh_last_error(); return; }
	}
	if (useMrf_) {                                                                                            // ... the MRF stage of all views side by side
		std::vector<int32_t> all(V);
		for (int v = 0; v < V; ++v) all[v] = v;
		if (srh_mvs_mrf_estimate_views(ctx_, all.data(), V, &mrfParams_, nullptr) != SRH_OK) { error_ = srh_last_error(); return; }
	}
	if (useSgm_) {                                                                                            // the aggregation in its place
		std::vector<int32_t> all(V);
		for (int v = 0; v < V; ++v) all[v] = v;
		sgmInfos_.assign(V, srh_sgm_info());
		if (srh_mvs_sgm_estimate_views(ctx_, all.data(), V, &sgmParams_, sgmInfos_.data()) != SRH_OK) { error_ = srh_last_error(); return; }
	}
	if (subpixel_) {                                     // sub-pixel depth (not in the reference): every view's finished map, no step of its own
		subpixelInfos_.assign(V, srh_mvs_subpixel_info());
		for (int v = 0; v < V; ++v) {
			if (isCancelled()) return;
			if (srh_mvs_view_subpixel(ctx_, v, &neigh[static_cast<size_t>(v)*nn], count[v], &params_, &subpixelInfos_[v],
			                          nullptr, nullptr, nullptr, nullptr) != SRH_OK) { error_ = srh_last_error(); return; }
		}
	}
	for (int v = 0; v < V; ++v)
		if (srh_view_depth_download(ctx_, v, computedDepths[v].data()) != SRH_OK) { error_ = srh_last_error(); return; }
	emit stageUpdate(tr("Constructing depth maps"));
	for (int v = 0; v < V; ++v) colorize(v);
	emit stageUpdate(tr("Cross-checking"));
	for (int v = 0; v < V; ++v) {
		if (isCancelled()) return;
		emit progressUpdate(step++);
		if (srh_mvs_cross_check(ctx_, slotIds.data(), V, v, &params_) != SRH_OK) { error_ = srh_last_error(); return; }
	}
	if (speckleMinSize_ > 0) {                           // the speckle filter (not in the reference): NaN, as the cross-check rejects
		srh_speckle_params s;
		srh_speckle_params_defaults(&s);
		s.min_size = speckleMinSize_; s.max_diff = speckleMaxDiff_; s.flags = SRH_SPECKLE_TO_NAN;
		for (int v = 0; v < V; ++v) {
			if (isCancelled()) return;
			if (srh_view_filter_speckles(ctx_, v, &params_, &s, nullptr, nullptr) != SRH_OK) { error_ = srh_last_error(); return; }
		}
	}
	for (int v = 0; v < V; ++v)
		if (srh_view_depth_download(ctx_, v, computedDepths[v].data()) != SRH_OK) { error_ = srh_last_error(); return; }
	emit stageUpdate(tr("Constructing depth maps"));
	for (int v = 0; v < V; ++v) colorize(v);
}

std::vector<FusedPoint> MultiViewStereo::fusedPointCloud() {
	std::vector<FusedPoint> pts;
	const int V = static_cast<int>(views_.size());
	if (!ctx_ || V == 0) return pts;
	params_.min_depth = minDepth; params_.max_depth = maxDepth; params_.num_depth_levels = numDepthLevels;
	params_.image_scale = imageScale; params_.cross_check_threshold = crossCheckThreshold;
	std::vector<int32_t> slotIds(V);
	for (int v = 0; v < V; ++v) {
		slotIds[v] = v;
		if (srh_view_depth_upload(ctx_, v, computedDepths[v].data()) != SRH_OK) { error_ = srh_last_error(); return pts; }
	}
	int64_t n = 0;
	if (srh_mvs_fuse(ctx_, slotIds.data(), V, &params_, &fuseParams_, nullptr) != SRH_OK ||
	    srh_mvs_fused_count(ctx_, &n) != SRH_OK) { error_ = srh_last_error(); return pts; }
	const size_t k = static_cast<size_t>(n);
	std::vector<double> xyz(3*k), nrm(3*k);
	std::vector<unsigned char> rgb(3*k), nviews(k), flags(k);
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

QImage MultiViewStereo::depthMap(CameraPtr view) const {
	for (size_t v = 0; v < views_.size(); ++v)
		if (views_[v].ptr && views_[v].ptr == view) return results[v];
	return QImage();
}

QImage MultiViewStereo::depthMap(const QString &viewId) const {
	for (size_t v = 0; v < views_.size(); ++v)
		if (views_[v].id == viewId) return results[v];
	return QImage();
}
