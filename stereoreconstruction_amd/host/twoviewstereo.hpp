// twoviewstereo.hpp -- TwoViewStereo with the reference's public interface
// (stereo/twoviewstereo.hpp:39-126), running on libstereo_recon_hip (MI355X).
// Differences forced by dropping Qt: QImage -> Image (already scaled by imageScale),
// QString -> std::string, signals -> std::function members of Task.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "camera.hpp"
#include "image.hpp"
#include "task.hpp"

class TwoViewStereo : public Task {
public:
	typedef std::vector<double> DepthMap;

	TwoViewStereo(CameraPtr leftView, Image left, Image leftMask,
	              CameraPtr rightView, Image right, Image rightMask,
	              double minDepth, double maxDepth,
	              int numDepthLevels,
	              double imageScale = 1.0,
	              int deviceOrdinal = 0);
	// The reference's constructor as it is called (twoviewstereo.cpp:89-124): images and mask images at FILE RESOLUTION,
	// smooth-scaled here, on the device, in Qt's arithmetic (srh_view_upload_scaled, SRH_MASK_IMAGE_SMOOTH) --
	// each image by width*imageScale, each mask image by its own; a null mask image: all WHITE.  Image::hasAlpha says which
	// of Qt's two 32-bit formats the file decoded to.  A shape the library does not scale leaves lastError() set and the
	// object without images (computeDepthMaps then fails the way it does without a device).
	struct ScaleOnDevice { };
	TwoViewStereo(ScaleOnDevice, CameraPtr leftView, const Image &left, const Image &leftMask,
	              CameraPtr rightView, const Image &right, const Image &rightMask,
	              double minDepth, double maxDepth,
	              int numDepthLevels,
	              double imageScale = 1.0,
	              int deviceOrdinal = 0);
	~TwoViewStereo();

	std::string title() const { return "Two-View Stereo"; }
	int numSteps() const { return 8; }

	void computeDepthMaps();

	// Hole filling after the cross-check (SRH_FILTER_* flags: 1 gaps, 2 weighted median, 3 both = filterInvalidPixels with
	// its #if 0 half).  0 (default) is the reference, whose call site is under #if 0 (twoviewstereo.cpp:200-223).
	void setFilterInvalid(int flags) { filterFlags = flags; }
	int filterInvalid() const { return filterFlags; }

	// Speckle filter between the cross-check and the hole filling (NOT IN THE REFERENCE; srh_view_filter_speckles): the
	// 4-connected components of valid pixels whose depths differ by at most diffSteps depth steps, those smaller than
	// minSize set to +INF in both maps (options "speckle_min_size" / "speckle_diff_steps").  0 (default): off.
	void setSpeckleFilter(int minSize, int diffSteps = 2) { speckleMinSize = minSize; speckleDiffSteps = diffSteps; }
	int speckleFilter() const { return speckleMinSize; }

	// Matching cost of the WTA: SRH_COST_NCC (0, default: cost_ncc, as the reference's computeCostVolumes) or SRH_COST_SAD
	// (1: cost_sad, twoviewstereo.cpp:864-905) or SRH_COST_CENSUS (3: the support-weighted census cost, not in the
	// reference).  The WTA, ratio test, cross-check and hole filling are the same for all.
	void setCostFunction(int kind) { costKind = kind; }
	int costFunction() const { return costKind; }
	// SAD of a rectified pair on the dense plan (option "sad_dense": 1 = on, 0 = default): a tuning switch, never the result
	void setSadDense(int on) { sadDenseOn = on; }
	int sadDense() const { return sadDenseOn; }
	// the census cost of a rectified pair on the dense plan (option "census_dense": 1 = on, 0 = default): likewise
	void setCensusDense(int on) { censusDenseOn = on; }
	int censusDense() const { return censusDenseOn; }

	// By-products of the WTA scan (option "wta_outputs"; never the depth maps): SRH_WTA_WINNERS (1) keeps, per pixel of each
	// map, the candidate pixel of the other view that won and the one that held the minimum before it (its cost is the
	// ratio test's secondBest); SRH_WTA_WINNERS | SRH_WTA_COSTS (3) also their costs in the reference's arithmetic.  0
	// (default): nothing is kept.  After computeDepthMaps(): (x, y) pairs, (-1, -1) = none; costs, +INF = none.  Empty
	// vectors when the outputs were not kept, or under setUseMRF(true) / setUseSGM(true) (no scan makes those maps).
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

	// Rectification (NOT IN THE REFERENCE; stereo_recon_hip.h): off (default) nothing changes.  On,
	// computeDepthMaps uploads the views as ever (slots 0, 1), warps them onto a rectified pair of cameras (slots 2, 3:
	// srh_twoview_rectify with rectifyParams()), runs the whole configured pipeline on the rectified pair -- WTA or SGM or MRF,
	// cross-check, speckles, hole filling -- where a verged, distorted pair gets the row-aligned dense plan, and brings both
	// depth maps back (srh_view_depth_unrectify): leftDepths(), rightDepths() and the colourised maps stay in the views the
	// caller handed in, at their size.  The rectified products are kept beside them: the rectified depth maps (z along the
	// rectified axis), images (rectifiedLeftMaskBytes(): 1 = WHITE) and cameras, all of rectifyParams().out_w x out_h
	// pixels (0: the left image's size), and what srh_twoview_rectify reported.  The WTA by-products of setKeepWtaOutputs,
	// when kept, are in RECTIFIED coordinates: pixels of the rectified views, rectified size.  A pair the library refuses to
	// rectify (a refractive camera, a baseline along the viewing direction, coincident centres) sets lastError() and runs
	// unrectified: rectified() then says false and the rectified products are empty.
	void setRectify(bool on) { rectifyOn = on; }
	bool rectify() const { return rectifyOn; }
	srh_rectify_params &rectifyParams() { return rectParams_; }   // focal, principal point, output size, SRH_RECTIFY_SHARED_CX
	bool rectified() const { return rectified_; }                  // the last computeDepthMaps ran on the rectified pair
	const DepthMap &rectifiedLeftDepths() const { return rectDepth_[0]; }
	const DepthMap &rectifiedRightDepths() const { return rectDepth_[1]; }
	const Image &rectifiedLeftImage() const { return rectImage_[0]; }
	const Image &rectifiedRightImage() const { return rectImage_[1]; }
	const std::vector<uint8_t> &rectifiedLeftMaskBytes() const { return rectMask_[0]; }
	const std::vector<uint8_t> &rectifiedRightMaskBytes() const { return rectMask_[1]; }
	const srh_camera &rectifiedCamera(bool left = true) const { return rectCam_[left ? 0 : 1]; }
	const srh_rectify_info &rectifyInfo() const { return rectInfo_; }

	// The MRF stage (a USE_MRF build of the reference, twoviewstereo.cpp:240-258, 308-403, 504-570; PARITY UNPINNED, see
	// stereo_recon_hip.h): off (default) computeDepthMaps is the WTA of the reference as it is compiled; on, each direction's
	// depth map comes from TRW-S over the full label cost volume (srh_twoview_compute_mrf: progress 1, 2 "Optimizing...",
	// 3, 4 "Optimizing...", 5, 8), the cross-check and the optional hole filling unchanged.  numSteps() stays 8.
	void setUseMRF(bool on) { useMrf = on; if (on) useSgm = false; }
	bool useMRF() const { return useMrf; }
	srh_twoview_mrf_params &mrfParams() { return mrfParams_; }     // SMOOTHNESS_EXP / _MAX / _LAMBDA, 50 sweeps, drop 5
	// what the optimiser of the last computeDepthMaps reported for the left / right map (iterations 0: none ran)
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

	// Candidate pixels, in visiting order, of pixel (x,y) of the left (fromLeft) or right view in the
	// other view.  The reference's public epipolarCurve (twoviewstereo.hpp:66-70) takes the unprojected
	// ray, camera offset, plane normal, mask and view; all of them follow from the pixel and the
	// direction, which is what StereoWidget has in hand (stereowidget.cpp:621-672).
	std::vector<std::pair<int, int> > epipolarCurve(int x, int y, bool fromLeft = true);

	// the scaled images and masks (1 = WHITE) computeDepthMaps uploads
	const Image &leftImage() const { return left; }
	const Image &rightImage() const { return right; }
	const std::vector<uint8_t> &leftMaskBytes() const { return leftMask; }
	const std::vector<uint8_t> &rightMaskBytes() const { return rightMask; }

	Image leftDepthMap() const { return resultLeft; }
	Image rightDepthMap() const { return resultRight; }

	// raw results (computedDepthLeft / computedDepthRight of the reference, twoviewstereo.hpp:113-114)
	const DepthMap &leftDepths() const { return computedDepthLeft; }
	const DepthMap &rightDepths() const { return computedDepthRight; }

	srh_params &params() { return params_; }          // every hard-coded constant, with the reference's defaults
	const std::string &lastError() const { return error_; }

protected:
	void runTask() { computeDepthMaps(); }

	// the reference's protected stages (twoviewstereo.hpp:72-84), for subclasses that re-sequence them:
	// WTA of both directions into computedDepthLeft/Right (twoviewstereo.cpp:233-501, non-MRF body) ...
	void computeCostVolumes(CameraPtr leftView, CameraPtr rightView);
	// ... and the mutual consistency filter on them (:596-672)
	void crossCheck(CameraPtr leftView, CameraPtr rightView);
	// label -> depth, non-uniform (:981-985)
	double depthFromLabel(int label) const;
	// ... and the hole filling of both maps (:676-767, progress 6): the compiled body, the row gap fill -- or, after
	// setFilterInvalid, what its flags ask for (with the median: also progress 7 and the #if 0 half, :769-810).
	// (weightedMedian is per pixel and stateful on the reference's weightFuncs: the device does it inside
	// filterInvalidPixels.)
	void filterInvalidPixels();
	// ... and, for a subclass that wants it between the two, the speckle filter of setSpeckleFilter on both maps (nothing
	// when that is off): uploads both maps, filters, downloads both, as filterInvalidPixels does
	void filterSpeckles();
	// the two matching costs (twoviewstereo.hpp:92-99) of reference pixel (x1,y1) against (x2,y2) of the other view.  The
	// reference passes the two images and masks and reads the window of weightFuncs, which init_weights has set for
	// (x1,y1) beforehand; as with epipolarCurve, all of that follows from the pixels and the direction: fromLeft = the
	// left view is the reference, else the right one.  The window is built on the device for each call (one round trip:
	// srh_twoview_pair_costs takes many pairs at once).  NaN when the device call fails (lastError()).
	double cost_sad(int x1, int y1, int x2, int y2, bool fromLeft = true);
	// (not in the reference: the census cost of option "cost" = SRH_COST_CENSUS, same conventions)
	double cost_census(int x1, int y1, int x2, int y2, bool fromLeft = true);
	double cost_ncc(int x1, int y1, int x2, int y2, bool fromLeft = true);

private:
	bool uploadViews();
	void setUp(int deviceOrdinal);
	double pairCost(int kind, int x1, int y1, int x2, int y2, bool fromLeft);
	void fetchWtaOutputs(int leftSlot = 0, int rightSlot = 1);
	bool rectifyViews();
	bool unrectifyMaps();
	void colorize(const DepthMap &d, Image &out) const;
	void colorFromDepth(double depth, uint8_t rgb[3]) const;

	CameraPtr leftView, rightView;
	Image left, right;
	std::vector<uint8_t> leftMask, rightMask;
	double minDepth, maxDepth;
	int numDepthLevels;
	double imageScale;
	Image resultLeft, resultRight;
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
	Image rectImage_[2];
	std::vector<uint8_t> rectMask_[2];
	srh_context *ctx_;
	std::string error_;
};
