// multiviewstereo.hpp -- MultiViewStereo with the reference's public interface
// (stereo/multiviewstereo.hpp:36-113) on libstereo_recon_hip.  initialize() takes the views'
// already-loaded, already-scaled images instead of (ProjectPtr, ImageSetPtr): the project /
// image-set data model is out of scope and only its outputs --
// camera parameters and pixels -- feed this path.
#pragma once

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "camera.hpp"
#include "image.hpp"
#include "project.hpp"
#include "task.hpp"

struct PLYPoint { double p[3]; uint8_t rgb[3]; };
void outputPLYFile(const std::string &path, const std::vector<PLYPoint> &points);   // multiviewstereo.cpp:291-315
// One point of the fused cloud (srh_mvs_fuse): position, unit normal, colour, the number of views that agree on it, flags
// (bit 0: the normal comes from the surface, else it points at the camera), and where it comes from: the index of the view
// in the run and the pixel index y*w + x in that view.
struct FusedPoint { double p[3], n[3]; uint8_t rgb[3], nviews, flags; int view, pixel; };
// The same file with normals: the header of the overload above with "property float nx", "ny", "nz" between z and the
// colours, lines "x y z nx ny nz r g b" -- what the reference's viewer reads (gui/mainwindow.cpp:304-461), which otherwise
// sets every normal to (0, 0, 1).
void outputPLYFile(const std::string &path, const std::vector<FusedPoint> &points);

class MultiViewStereo : public Task {
public:
	typedef std::vector<double> DepthMap;

	explicit MultiViewStereo(int deviceOrdinal = 0);
	~MultiViewStereo();

	// images[i] is the default image of views[i] scaled by imageScale; its alpha channel is the
	// mask (alpha == 255 <=> WHITE, multiviewstereo.cpp:225-234).  Views with a null image are skipped.
	void initialize(const std::vector<CameraPtr> &views, const std::vector<Image> &images,
	                double minDepth, double maxDepth,
	                int numDepthLevels,
	                double crossCheckThreshold,
	                double imageScale = 1.0);

	// The reference's own signature (multiviewstereo.hpp:46-52): views are looked up in `imageSet` (default image
	// per camera; cameras without one, or whose file `load` cannot produce, are skipped, :218-220).  Decoding and
	// the two Qt scalings stay with the caller: load(file, imageScale, image, maskSource) returns the
	// smooth-scaled image and -- when the file has an alpha channel -- the fast-scaled copy the mask is taken from
	// (maskSource left null: all pixels WHITE, :225-237).
	typedef std::function<bool(const std::string &file, double imageScale, Image &image, Image &maskSource)> ImageLoader;
	void initialize(ProjectPtr project, ImageSetPtr imageSet, const std::vector<CameraPtr> &views,
	                double minDepth, double maxDepth,
	                int numDepthLevels,
	                double crossCheckThreshold,
	                double imageScale,
	                const ImageLoader &load);
	// The same with the scaling done HERE, on the device, in Qt's arithmetic (srh_view_upload_scaled, SRH_MASK_ALPHA_FAST;
	// DESIGN.md 4f): decode(file, image) returns the file's pixels undecorated, at file resolution, with image.hasAlpha set;
	// the smooth-scaled image and the mask of the fast-scaled copy's alpha come back from the device.  A view whose file
	// `decode` cannot produce is skipped; one whose shape the library does not scale is skipped with lastError() set.
	typedef std::function<bool(const std::string &file, Image &image)> ImageDecoder;
	void initialize(ProjectPtr project, ImageSetPtr imageSet, const std::vector<CameraPtr> &views,
	                double minDepth, double maxDepth,
	                int numDepthLevels,
	                double crossCheckThreshold,
	                double imageScale,
	                const ImageDecoder &decode);
	ImageSetPtr imageSet() const { return imageSet_; }   // the image set of the last initialize (multiviewstereo.hpp:62)

	std::string title() const { return "Multi-View Stereo"; }
	int numSteps() const;                              // 2 * views (multiviewstereo.cpp:319-321)

	Image depthMap(CameraPtr view) const;              // grayscale, NaN/INF/unknown white (:252-276)
	const DepthMap *depths(CameraPtr view) const;      // computedDepths[view]
	// The view's current depth map as coloured 3-D points (pixels with a WHITE mask and a finite depth; the point
	// is the cross-checks' construction, multiviewstereo.cpp:688-692) -- what outputPLYFile takes.
	std::vector<PLYPoint> pointCloud(CameraPtr view);
	// The depth maps of all views of the last run, in their order, fused into one oriented cloud (srh_mvs_fuse with
	// fuseParams(); not in the reference): every surface patch once, with the views that confirm it averaged;
	// by default (min_views 2) points no second view confirms are left out.  Empty with lastError() set when it fails.
	std::vector<FusedPoint> fusedPointCloud();
	srh_fuse_params &fuseParams() { return fuseParams_; }
	// "percent of pixels have depth hypotheses": finite depths among the masked-in pixels (:402-421)
	double coverage(CameraPtr view) const;
	const std::vector<std::vector<int> > &neighbourViews() const { return neighbours; }
	// what initialize() kept for the view, as runTask uploads it: the scaled pixels and the mask bytes (1 = WHITE); null when
	// the view is not part of the run
	const Image *image(CameraPtr view) const;
	const std::vector<uint8_t> *mask(CameraPtr view) const;

	srh_params &params() { return params_; }
	// The reference picks the MRF branch of computeInitialEstimate at build time (CONFIG+=mrf -> USE_MRF,
	// StereoReconstruction.pro:100-103); here it is a run-time switch, off by default like the reference's default build.
	void setUseMRF(bool on) { useMrf_ = on; if (on) useSgm_ = false; }
	bool useMRF() const { return useMrf_; }
	srh_mrf_params &mrfParams() { return mrfParams_; }
	// Semi-global aggregation over the peak labels (srh_mvs_sgm_estimate_views; not in the reference): one
	// pass along the directions of sgmParams().path_mask where the MRF branch sweeps until its energy settles.  Off by
	// default; setUseSGM(true) and setUseMRF(true) switch each other off (the last call wins).  sgmInfo(view): the
	// directions aggregated and the labelling's MRF energy of the last run (paths 0 before one, or for an unknown view).
	void setUseSGM(bool on) { useSgm_ = on; if (on) useMrf_ = false; }
	bool useSGM() const { return useSgm_; }
	srh_mvs_sgm_params &sgmParams() { return sgmParams_; }
	srh_sgm_info sgmInfo(CameraPtr view) const;
	// Sub-pixel depth (NOT IN THE REFERENCE; srh_mvs_view_subpixel): every view's map is refined after its
	// estimate -- the WTA's, setUseMRF's or setUseSGM's -- with the neighbour list the estimate used, before the cross-check
	// and the speckle filter.  Off by default: the maps are the reference's.  The step count is unchanged.
	// subpixelInfo(view): the pixels per class of the last run (all zero before one, with the stage off, or for an unknown view).
	void setSubpixel(bool on) { subpixel_ = on; }
	bool subpixel() const { return subpixel_; }
	srh_mvs_subpixel_info subpixelInfo(CameraPtr view) const;
	// Speckle filter after the cross-check (NOT IN THE REFERENCE; srh_view_filter_speckles with SRH_SPECKLE_TO_NAN): in
	// every view's map the 4-connected components of valid pixels whose depths differ by at most maxDiff (<= 0: two depth
	// steps), those smaller than minSize set to NaN -- before depthMap, pointCloud and fusedPointCloud read the maps.
	// 0 (default): off.  The step count is unchanged.
	void setSpeckleFilter(int minSize, double maxDiff = 0) { speckleMinSize_ = minSize; speckleMaxDiff_ = maxDiff; }
	int speckleFilter() const { return speckleMinSize_; }
	const std::string &lastError() const { return error_; }

protected:
	void runTask();

private:
	void colorize(size_t v);

	ProjectPtr project;
	ImageSetPtr imageSet_;
	std::vector<CameraPtr> views;
	std::vector<Image> images;
	std::vector<std::vector<uint8_t> > masks;
	std::vector<Image> results;
	std::vector<DepthMap> computedDepths;
	std::vector<std::vector<int> > neighbours;
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
	std::string error_;
};
