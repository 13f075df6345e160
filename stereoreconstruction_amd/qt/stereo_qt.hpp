// stereo_qt.hpp -- the Qt binding of libstereo_recon_hip: TwoViewStereo and MultiViewStereo with the reference's OWN
// public signatures (stereo/twoviewstereo.hpp:39-70, stereo/multiviewstereo.hpp:44-63), derived from the reference's own
// Task (gui/task.hpp:57-105; compiled from /root/reference where it lies, with its moc output), QImage in and out, the
// reference's signals, everything between "scaled images + cameras" and "depth maps" behind the C-ABI.
//
// Camera / Project / ImageSet / Ray3d / VectorImage / Eigen::Vector3d appear here as FORWARD DECLARATIONS only, exactly
// as stereo/*.hpp forward-declare the first three (FORWARD_DECLARE, util/precompiled.hpp:60-63): the binding never looks
// inside them.  What it needs from them -- a POD snapshot of a camera, its id and name, the image file an image set holds
// for a camera, the pixel a curve query is about -- comes through the glue declared below (srq::cameraInfo,
// srq::defaultImageFile, and the definition of the five-argument TwoViewStereo::epipolarCurve), defined in ONE translation
// unit of the host application:
//   qt/glue_reference.cpp   for the reference itself (includes project/camera.hpp, project/imageset.hpp, util/ray.hpp:
//                           needs Eigen and OpenCV, which this image lacks, so it is compiled where they exist;
//                           INTEGRATION.md shows it in full),
//   tests/qt_glue_test.hpp  the test driver's own small Camera / ImageSet / ... classes.
// gui/widgets/stereowidget.cpp's call sites (:160, 263, 274, 321-322, 964-966, 990-994) compile against this header
// unchanged; tests/qt_adapter_test.cpp holds them as a type-check.
#pragma once

#include <QtCore/QString>
#include <QtGui/QImage>

#include <array>
#include <string>
#include <utility>
#include <vector>

#include <memory>

#include "gui/task.hpp"                 // the reference's Task (QObject with run/cancel slots and progress signals)
#include "stereo_recon_hip.h"

FORWARD_DECLARE(Project);               // class Project; typedef std::shared_ptr<Project> ProjectPtr; ... (the reference's macro)
FORWARD_DECLARE(Camera);
FORWARD_DECLARE(ImageSet);
class Ray3d;
class VectorImage;
struct RGBA;                            // util/vectorimage.hpp:28
namespace Eigen {
template <typename Scalar, int Rows, int Cols, int Options, int MaxRows, int MaxCols> class Matrix;   // (Eigen's own forward declaration, minus its defaults)
typedef Matrix<double, 3, 1, 0, 3, 1> Vector3d;
}

// stereo/multiviewstereo.hpp:36-39, verbatim but for Ray3d::Point spelt as what it is (util/ray.hpp:32: Eigen::Vector3d).
// Both are incomplete types here; outputPLYFile is DEFINED in the glue translation unit, over srq::writePLY below.
typedef std::pair<Eigen::Vector3d, RGBA> PLYPoint;
//! Output a set of points to a PLY file
void outputPLYFile(const std::string &path, const std::vector<PLYPoint> &points);

// One point of the fused cloud (srh_mvs_fuse; not in the reference): position, unit normal, colour, the number
// of views that agree on it, flags (bit 0: the normal comes from the surface), the view's index in the run and the pixel.
struct FusedPoint { double p[3], n[3]; unsigned char rgb[3], nviews, flags; int view, pixel; };
// the PLY file with normals ("x y z nx ny nz r g b", the properties nx, ny, nz between z and the colours): what the
// reference's viewer reads (gui/mainwindow.cpp:304-461)
void outputPLYFile(const std::string &path, const std::vector<FusedPoint> &points);

namespace srq {

// the text outputPLYFile writes (multiviewstereo.cpp:291-315): ASCII header, then "x y z r g b" per point through
// operator<< of an ofstream; xyz = 3 doubles per point, rgb = 3 bytes per point (the reference prints static_cast<int>(rgb.r))
void writePLY(const std::string &path, size_t npoints, const double *xyz, const unsigned char *rgb);
// the same with the colours as the ints the reference prints: its RGBA holds doubles and static_cast<int>(rgb.r) goes out
// unchanged -- a component outside 0 .. 255 (or negative) must not wrap modulo 256 on the way (outputPLYFile uses this one)
void writePLY(const std::string &path, size_t npoints, const double *xyz, const int *rgb);

// VectorImage::fromQImage (util/vectorimage.cpp:48-64): the raw 32-bit scanline words as R,G,B,A bytes.  (A smooth-
// scaled ARGB32 image is ARGB32_Premultiplied; the reference reads it raw, and so does this.)  Images that are not
// 32 bits deep, which the reference would misread, are converted to ARGB32 first.
struct Raster { int w = 0, h = 0; std::vector<unsigned char> rgba; };
Raster rasterFromQImage(const QImage &img);
// mask.pixel(x,y) == WHITE for every pixel of a mask image (util/vectorimage.hpp:64-69): 1 where r=g=b=a=255
std::vector<unsigned char> whiteMask(const Raster &mask);
// the image + mask MultiViewStereo::initialize builds from a file (multiviewstereo.cpp:216-241): smooth-scaled image;
// mask = alpha == 255 on a FAST-scaled copy when the file has an alpha channel, all WHITE otherwise
bool ingestViewFile(const QString &file, double imageScale, Raster &image, std::vector<unsigned char> &mask);

// ---- the glue: DECLARED here, DEFINED by the host application (see the header comment) ----
struct CameraInfo { srh_camera camera; QString id, name; };
// K, R, t, distortion, refractive interface of a project camera as the POD the C-ABI takes (a copy, not a live pointer)
CameraInfo cameraInfo(const Camera &cam);
// imageSet->defaultImageForCamera(cam)->file(), empty when the set has no image for the camera (multiviewstereo.cpp:214)
QString defaultImageFile(const ImageSet &set, const CameraPtr &cam);

} // namespace srq

class TwoViewStereo : public Task {
public:
	typedef std::vector<double> DepthMap;

	// stereo/twoviewstereo.hpp:44-47, verbatim.  The GPU is chosen with setDevice() (default 0).
	TwoViewStereo(CameraPtr leftView, QImage left, QImage leftMask,
	              CameraPtr rightView, QImage right, QImage rightMask,
	              double minDepth, double maxDepth, int numDepthLevels,
	              double imageScale = 1.0);
	~TwoViewStereo();
	static void setDevice(int ordinal);

	QString title() const { return "Two-View Stereo"; }
	int numSteps() const { return 8; }

	void computeDepthMaps();
	QImage leftDepthMap() const { return resultLeft; }
	QImage rightDepthMap() const { return resultRight; }
	// stereo/twoviewstereo.hpp:66-70, verbatim (twoviewstereo.cpp:999-1054): the candidate pixels (tx, ty, 1) of the
	// reference pixel whose `ray` this is, in the order the reference visits them, joint duplicates included.  Every
	// caller builds (ray, cameraOffset, depthPlaneNormal, mask, view) from a pixel of one view the same way
	// (twoviewstereo.cpp:275-283, 445-453: ray = unproject((x + 0.5)/scale, (y + 0.5)/scale), offset and normal of the same
	// camera, mask and `view` of the other one), so the glue translation unit -- which knows Ray3d and Eigen -- recovers
	// the pixel and the direction and calls curveOfPixel(); that is where this member is DEFINED.
	std::vector<Eigen::Vector3d> epipolarCurve(const Ray3d &ray,
	                                           const Eigen::Vector3d &cameraOffset,
	                                           const Eigen::Vector3d &depthPlaneNormal,
	                                           const VectorImage &mask,
	                                           CameraPtr view) const;

	// ---- beyond the reference's interface ----
	std::vector<std::array<double, 3> > curveOfPixel(int x, int y, bool fromLeft = true) const;
	CameraPtr leftCamera() const { return leftView; }
	CameraPtr rightCamera() const { return rightView; }
	double scale() const { return imageScale; }
	const DepthMap &leftDepths() const { return computedDepthLeft; }
	const DepthMap &rightDepths() const { return computedDepthRight; }
	srh_params &params() { return params_; }
	QString lastError() const { return error_; }
	// hole filling after the cross-check (SRH_FILTER_* flags); 0 (default) = the reference, call site under #if 0
	void setFilterInvalid(int flags) { filterFlags = flags; }
	// speckle filter between the cross-check and the hole filling (not in the reference; srh_view_filter_speckles): components
	// of fewer than minSize pixels whose depths chain within diffSteps depth steps become +INF; 0 (default) = off
	void setSpeckleFilter(int minSize, int diffSteps = 2) { speckleMinSize = minSize; speckleDiffSteps = diffSteps; }
	// matching cost of the WTA: SRH_COST_NCC (0, default: cost_ncc, the reference's), SRH_COST_SAD (1: cost_sad) or
	// SRH_COST_CENSUS (3: the support-weighted census cost, not in the reference)
	void setCostFunction(int kind) { costKind = kind; }
	int costFunction() const { return costKind; }
	// SAD of a rectified pair on the dense plan (option "sad_dense": 1 = on, 0 = default): a tuning switch, never the result
	void setSadDense(int on) { sadDenseOn = on; }
	int sadDense() const { return sadDenseOn; }
	// the census cost of a rectified pair on the dense plan (option "census_dense": 1 = on, 0 = default): likewise
	void setCensusDense(int on) { censusDenseOn = on; }
	int censusDense() const { return censusDenseOn; }
	// by-products of the WTA scan (option "wta_outputs"; never the depth maps): SRH_WTA_WINNERS (1) keeps per pixel of each map
	// the winning candidate pixel of the other view and the one that held the minimum before it, SRH_WTA_WINNERS |
	// SRH_WTA_COSTS (3) also their costs in the reference's arithmetic; 0 (default) nothing.  After computeDepthMaps(): (x, y)
	// pairs, (-1, -1) = none; costs, +INF = none.  Empty when nothing was kept, or under setUseMRF(true).
	void setKeepWtaOutputs(int flags) { wtaFlags = flags; }
	int keepWtaOutputs() const { return wtaFlags; }
	const std::vector<int32_t> &leftWinners() const { return winners_[0]; }
	const std::vector<int32_t> &leftRunnersUp() const { return runners_[0]; }
	const std::vector<double> &leftMinCosts() const { return minCosts_[0]; }
	const std::vector<double> &leftSecondCosts() const { return secondCosts_[0]; }
	const std::vector<int32_t> &rightWinners() const { return winners_[1]; }
	const std::vector<int32_t> &rightRunnersUp() const { return runners_[1]; }
	const std::vector<double> &rightMinCosts() const { return minCosts_[1]; }
	const std::vector<double> &rightSecondCosts() const { return secondCosts_[1]; }

	// Sub-pixel depth (NOT IN THE REFERENCE; option "subpixel", stereo_recon_hip.h): off (default) nothing
	// changes.  On, each WTA pass refines its map before the cross-check: a parabola through the costs of the winner and of
	// its two neighbours on the pixel's curve places the match between two pixels of the other view, and the depth is
	// triangulated there.  After computeDepthMaps(): delta per pixel of each map (0 where the pixel was not refined; > 0
	// towards the neighbour of larger depth), in RECTIFIED coordinates and size under setRectify, as the winners are.  Empty
	// vectors when the option is off, or under setUseMRF(true) / setUseSGM(true) (no scan makes those maps).
	void setSubpixel(bool on) { subpixelOn = on; }
	bool subpixel() const { return subpixelOn; }
	const std::vector<double> &leftSubpixelDelta() const { return subDelta_[0]; }
	const std::vector<double> &rightSubpixelDelta() const { return subDelta_[1]; }
	// the MRF stage (a USE_MRF build of the reference; PARITY UNPINNED, stereo_recon_hip.h): off (default) = the WTA; on, each
	// map comes from TRW-S over the label cost volume (srh_twoview_compute_mrf: progress 1, 2 "Optimizing...", 3, 4, 5, 8),
	// cross-check and optional hole filling unchanged.  Cancellation is observed at every progress step.
	void setUseMRF(bool on) { useMrf = on; if (on) useSgm = false; }
	bool useMRF() const { return useMrf; }
	srh_twoview_mrf_params &mrfParams() { return mrfParams_; }
	const srh_mrf_info &mrfInfo(bool left = true) const { return mrfInfo_[left ? 0 : 1]; }

	// Semi-global aggregation (NOT IN THE REFERENCE; stereo_recon_hip.h): between the WTA and the MRF stage --
	// each direction's depth map comes from one pass along up to 8 path directions over the label cost volume, with the MRF
	// stage's smoothness term (srh_twoview_compute_sgm: progress 1, 2 "Aggregating...", 3, 4 "Aggregating...", 5, 8), the
	// cross-check and the optional hole filling unchanged.  One of the two switches at most is on: the last call wins.
	void setUseSGM(bool on) { useSgm = on; if (on) useMrf = false; }
	bool useSGM() const { return useSgm; }
	srh_twoview_sgm_params &sgmParams() { return sgmParams_; }     // smoothness term 1 / 2 / 0.25, path_mask 0xFF
	// what the aggregation of the last computeDepthMaps reported for the left / right map (paths 0: none ran)
	const srh_sgm_info &sgmInfo(bool left = true) const { return sgmInfo_[left ? 0 : 1]; }

	// Rectification (NOT IN THE REFERENCE; stereo_recon_hip.h): off (default) nothing changes.  On, the views
	// are warped onto a rectified pair of cameras (srh_twoview_rectify with rectifyParams(), slots 2, 3), the whole configured
	// pipeline -- WTA or SGM or MRF, cross-check, speckles, hole filling; sequenced by the library, which reports the steps
	// through its hook -- runs on the rectified pair, where a verged, distorted pair gets the row-aligned dense plan, and
	// both depth maps come back (srh_view_depth_unrectify): leftDepths(), rightDepths(), leftDepthMap() and rightDepthMap()
	// stay in the views the caller handed in.  The rectified depth maps (z along the rectified axis), images and cameras, of
	// rectifyParams().out_w x out_h pixels (0: the left image's size), are kept beside them.  The WTA by-products of
	// setKeepWtaOutputs, when kept, are in RECTIFIED coordinates.  A pair the library refuses to rectify (a refractive
	// camera, a baseline along the viewing direction) sets lastError() and runs unrectified: rectified() says false.
	void setRectify(bool on) { rectifyOn = on; }
	bool rectify() const { return rectifyOn; }
	srh_rectify_params &rectifyParams() { return rectParams_; }
	bool rectified() const { return rectified_; }
	const DepthMap &rectifiedLeftDepths() const { return rectDepth_[0]; }
	const DepthMap &rectifiedRightDepths() const { return rectDepth_[1]; }
	QImage rectifiedLeftImage() const { return rectImage_[0]; }
	QImage rectifiedRightImage() const { return rectImage_[1]; }
	const srh_camera &rectifiedCamera(bool left = true) const { return rectCam_[left ? 0 : 1]; }
	const srh_rectify_info &rectifyInfo() const { return rectInfo_; }
	void relayProgress(int step, const char *stage);       // (the library's progress hook lands here)

public: // Task implementation continued: public in the reference as well (stereo/twoviewstereo.hpp:50-52)
	void runTask() { computeDepthMaps(); }

protected:
	// stereo/twoviewstereo.hpp, protected: the compiled body (row gap fill of both maps, progress 6), or what
	// setFilterInvalid asks for (the median: progress 7 and the #if 0 half, twoviewstereo.cpp:769-810)
	void filterInvalidPixels();
	// the speckle filter of setSpeckleFilter on both maps (nothing when it is off), progress 5 "Removing speckles..."
	void filterSpeckles();
	// stereo/twoviewstereo.hpp:92-99, protected: cost_sad / cost_ncc of reference pixel (x1,y1) against (x2,y2) of the
	// other view.  The reference passes both images and masks and reads weightFuncs, set by init_weights for (x1,y1); as
	// with curveOfPixel all of it follows from the pixels and the direction (fromLeft: the left view is the reference).
	// One device round trip per call (srh_twoview_pair_costs takes many pairs); NaN when it fails (lastError()).
	double cost_sad(int x1, int y1, int x2, int y2, bool fromLeft = true);
	double cost_census(int x1, int y1, int x2, int y2, bool fromLeft = true);   // (not in the reference)
	double cost_ncc(int x1, int y1, int x2, int y2, bool fromLeft = true);

private:
	double pairCost(int kind, int x1, int y1, int x2, int y2, bool fromLeft);
	void fetchWtaOutputs(int leftSlot = 0, int rightSlot = 1);
	bool rectifyViews();
	QImage colorize(const DepthMap &d, int w, int h) const;
	CameraPtr leftView, rightView;
	srh_camera leftCam, rightCam;                          // snapshots taken by the constructor (srq::cameraInfo)
	srq::Raster left, right;
	std::vector<unsigned char> leftMask, rightMask;
	double minDepth, maxDepth;
	int numDepthLevels;
	double imageScale;
	QImage resultLeft, resultRight;
	DepthMap computedDepthLeft, computedDepthRight;
	srh_params params_;
	int filterFlags = 0;
	int speckleMinSize = 0, speckleDiffSteps = 2;
	int costKind = SRH_COST_NCC;
	int sadDenseOn = 0;
	int censusDenseOn = 0;
	int wtaFlags = 0;
	bool subpixelOn = false;
	std::vector<double> subDelta_[2];
	std::vector<int32_t> winners_[2], runners_[2];
	std::vector<double> minCosts_[2], secondCosts_[2];
	bool useMrf = false;
	srh_twoview_mrf_params mrfParams_;
	srh_mrf_info mrfInfo_[2];
	bool useSgm = false;
	srh_twoview_sgm_params sgmParams_;
	srh_sgm_info sgmInfo_[2];
	bool rectifyOn = false, rectified_ = false;
	srh_rectify_params rectParams_;
	srh_rectify_info rectInfo_;
	srh_camera rectCam_[2];
	DepthMap rectDepth_[2];
	QImage rectImage_[2];
	volatile int cancelWord_ = 0;                         // what the library polls: set from isCancelled() at progress steps
	srh_context *ctx_;
	mutable bool uploaded_ = false;                        // views resident on the device (epipolarCurve before computeDepthMaps)
	bool uploadViews() const;
	mutable QString error_;
};

class MultiViewStereo : public Task {
public:
	// a camera of the project, its snapshot and its image file: what initialize() resolves every CameraPtr into
	struct View { QString id, name; srh_camera camera; QString file; CameraPtr ptr; };

	MultiViewStereo();
	~MultiViewStereo();
	static void setDevice(int ordinal);

	// stereo/multiviewstereo.hpp:46-52, verbatim (multiviewstereo.cpp:193-247): loads, scales and masks the image the
	// image set holds for every view; views without an existing image file are skipped
	void initialize(ProjectPtr project,
	                ImageSetPtr imageSet,
	                const std::vector<CameraPtr> &views,
	                double minDepth, double maxDepth,
	                int numDepthLevels,
	                double crossCheckThreshold,
	                double imageScale = 1.0);
	// the same from resolved records (hosts without the reference's project model)
	void initialize(const std::vector<View> &views, double minDepth, double maxDepth, int numDepthLevels,
	                double crossCheckThreshold, double imageScale = 1.0);

	QString title() const { return "Multi-view Stereo"; }
	int numSteps() const { return 2*static_cast<int>(views_.size()); }

	QImage depthMap(CameraPtr view) const;                        // stereo/multiviewstereo.hpp:60; null image for an unknown view (:279-286)
	ImageSetPtr imageSet() const { return imageSet_; }            // stereo/multiviewstereo.hpp:63
	QImage depthMap(const QString &viewId) const;                 // (by id: record-based hosts)
	const std::vector<double> &depths(int viewIndex) const { return computedDepths[viewIndex]; }
	int numViews() const { return static_cast<int>(views_.size()); }
	const srq::Raster &image(int viewIndex) const { return images[viewIndex]; }
	const std::vector<unsigned char> &mask(int viewIndex) const { return masks[viewIndex]; }
	srh_params &params() { return params_; }
	// CONFIG+=mrf of the reference (USE_MRF, StereoReconstruction.pro:100-103) as a run-time switch; off by default
	void setUseMRF(bool on) { useMrf_ = on; if (on) useSgm_ = false; }
	srh_mrf_params &mrfParams() { return mrfParams_; }
	// Semi-global aggregation over the peak labels (NOT IN THE REFERENCE; stereo_recon_hip.h): one pass along
	// the directions of sgmParams().path_mask where the MRF branch sweeps (srh_mvs_sgm_estimate_views).  Off by default;
	// setUseSGM(true) and setUseMRF(true) switch each other off.  sgmInfo(viewIndex): paths and energy of the last run.
	void setUseSGM(bool on) { useSgm_ = on; if (on) useMrf_ = false; }
	bool useSGM() const { return useSgm_; }
	srh_mvs_sgm_params &sgmParams() { return sgmParams_; }
	srh_sgm_info sgmInfo(int viewIndex) const { return viewIndex >= 0 && viewIndex < static_cast<int>(sgmInfos_.size()) ? sgmInfos_[viewIndex] : srh_sgm_info(); }
	// the depth maps of the last run's views, in their order, fused into one oriented cloud (srh_mvs_fuse with fuseParams())
	std::vector<FusedPoint> fusedPointCloud();
	srh_fuse_params &fuseParams() { return fuseParams_; }
	// sub-pixel depth (NOT IN THE REFERENCE; srh_mvs_view_subpixel): every view's map is refined after its estimate
	// (WTA, setUseMRF or setUseSGM) with the estimate's neighbour list, before the cross-check and the speckle filter.  Off by
	// default; the step count is unchanged.  subpixelInfo(viewIndex): the pixels per class of the last run
	void setSubpixel(bool on) { subpixel_ = on; }
	bool subpixel() const { return subpixel_; }
	srh_mvs_subpixel_info subpixelInfo(int viewIndex) const { return viewIndex >= 0 && viewIndex < static_cast<int>(subpixelInfos_.size()) ? subpixelInfos_[viewIndex] : srh_mvs_subpixel_info(); }
	// speckle filter after the cross-check (not in the reference; srh_view_filter_speckles, SRH_SPECKLE_TO_NAN): components of
	// fewer than minSize pixels whose depths chain within maxDiff (<= 0: two depth steps) become NaN; 0 (default) = off
	void setSpeckleFilter(int minSize, double maxDiff = 0) { speckleMinSize_ = minSize; speckleMaxDiff_ = maxDiff; }
	QString lastError() const { return error_; }

protected:
	void runTask();

private:
	void colorize(int viewIndex);
	ProjectPtr project;
	ImageSetPtr imageSet_;
	std::vector<View> views_;
	std::vector<srq::Raster> images;
	std::vector<std::vector<unsigned char> > masks;
	std::vector<QImage> results;
	std::vector<std::vector<double> > computedDepths;
	double minDepth, maxDepth, crossCheckThreshold, imageScale;
	int numDepthLevels;
	srh_params params_;
	srh_mrf_params mrfParams_;
	srh_mvs_sgm_params sgmParams_;
	std::vector<srh_sgm_info> sgmInfos_;
	srh_fuse_params fuseParams_;
	bool useMrf_ = false, useSgm_ = false;
	bool subpixel_ = false;
	std::vector<srh_mvs_subpixel_info> subpixelInfos_;
	int speckleMinSize_ = 0;
	double speckleMaxDiff_ = 0;
	srh_context *ctx_;
	QString error_;
};
