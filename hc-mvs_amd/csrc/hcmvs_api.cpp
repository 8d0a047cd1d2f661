/*
 * hc-mvs_amd/csrc/hcmvs_api.cpp -- host side of the C-ABI declared in include/hcmvs_hip.h.
 *
 * Holds the per-device context (views resident in HBM, working maps, row-progress words), hands the
 * per-call constants of est_plan.h (DepthEstimator's constructor, DepthMap.cpp:386-439, DepthMap.h:412-444)
 * the device pointers and enqueues the kernels of pm_kernels.hip.  No compute happens on the host; without a usable HIP
 * device every entry point fails.
 */
#include "../../include/hcmvs_hip.h"
#include "pm_common.h"
#include "est_plan.h"
#include "fuse_common.h"
#include "pf_chain.h"
#include "filter_plan.h"
#include "fuse_plan.h"
#include "tri_init.h"
#include "cloud_kernels.h"
#include "vis_kernels.h"
#include "mesh_kernels.h"
#include "view_kernels.h"
#include "init_kernels.h"
#include "handoff_kernels.h"
#include "handoff_host.h"
#include "speckle_plan.h"
#include "speckle_host.h"
#include "speckle_kernels.h"
#include "prior_kernels.h"
#include "dev_buf.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <algorithm>
#include <chrono>
#include <vector>

using namespace hcmvs;

namespace {

constexpr int kMaxBatch = HCMVS_MAX_BATCH; // reference images estimated by one call
constexpr uint32_t kMaxViewId = 65536;      // view ids, and the ids a neighbour list may name, lie below it

struct View {
	View() = default;
	explicit View(Reclaimer* r) : grayMem(r), bgrMem(r), gra(r), keep(r), quads(r), depthMem(r), normalMem(r), confMem(r), dNeighbors(r), priorMem(r), region(r) {}
	int w = 0, h = 0;
	float* gray = nullptr;   // device: the caller's (hcmvs_set_view_device) or grayMem
	uint8_t* bgr = nullptr;  // device or null: the caller's or bgrMem
	DevBuf grayMem, bgrMem;  // the copies of hcmvs_upload_view
	DevBuf gra;              // gradient map, u8 (lazy)
	DevBuf keep;             // keep-mask of --ignore-mask-label, u8 per pixel (hcmvs_set_ignore_mask); empty = no mask
	DevBuf quads;            // float4: 2 x 2 footprint layout of the gray image, built when the view first serves as a source view
	double K[9], R[9], C[3];
	// estimated maps registered for filter / fuse: the caller's (hcmvs_set_depthmap_device) or the copies in *Mem
	float *mDepth = nullptr, *mNormal = nullptr, *mConf = nullptr;
	DevBuf depthMem, normalMem, confMem;
	float dMin = 0.f, dMax = 0.f;
	DevBuf dNeighbors; // uint32_t
	std::vector<uint32_t> neighbors;
	// --n-viewspread: the maps this view offers as a SOURCE view (hcmvs_set_spread_maps_device; the caller's, of the view's size)
	const float *sDepth = nullptr, *sNormal = nullptr, *sConf = nullptr;
	bool rescaled = false; // made by hcmvs_rescale_view: never spreads
	// depth prior of the view as a REFERENCE view, w * h floats: the caller's (hcmvs_set_depth_prior_device) or priorMem; null = none
	const float* prior = nullptr;
	DevBuf priorMem;
	DevBuf region;           // hcmvs_set_prior_region: u8 per pixel as the ignore-mask kernel writes it, 0 = INSIDE the region; empty = no region
};

} // namespace


// Every device buffer of the context gives the post-filter chain's state back when memory is short (the chain allocates it again, or
// falls back to fusions from scratch, the next time it runs) -- except that state itself.
struct hcmvs_ctx final : Reclaimer {
	int device = 0;
	hipStream_t ownStream = nullptr;
	hipStream_t stream = nullptr;
	std::string err;
	std::map<uint32_t, View> views;
	// working buffers of the batch items (grown on demand)
	struct Slot {
		explicit Slot(Reclaimer* r) : dn(r), conf(r), tmpDepth(r), progress(r), srcSlab(r) {}
		DevBuf dn, conf, tmpDepth; // float4, float, float per pixel
		DevBuf progress;           // int32_t, kProgressStride per row
		DevBuf srcSlab;            // compact copy of an item's source images when they are > 4 GiB apart
	};
	std::vector<Slot> slots;
	DevBuf tmpU8{this}; // gradient-map staging
	DevBuf maskStage{this}; // hcmvs_set_ignore_mask: the label image and the ignored labels on their way in
	// host-path staging
	DevBuf sDepth{this}, sNormal{this}, sConf{this};
	DevBuf dViews{this};                  // DevView [kMaxBatch][kViewSlotEntries]: an item's views, then its PriorItem (pm_types.h)
	std::vector<DevView> hViews;          // host copy handed to hipMemcpyAsync (must outlive the call)
	DevBuf dItems{this};                  // EstConst [kMaxBatch]
	std::vector<EstConst> hItems;
	DevBuf dSpread{this};                 // SpreadView [kMaxBatch][kMaxViews]
	std::vector<SpreadView> hSpread;
	int viewspread = 0;                   // hcmvs_set_viewspread
	bool haveSpreadStats = false;         // the last estimate ran with view spread in effect
	hcmvs_prior_params prior = {0.5f, 0.2f, 2}; // hcmvs_set_prior_params (the reference's defaults)
	bool havePriorStats = false;          // the last estimate had an item with an active prior
	hcmvs_geo_params geo = {0, 0.25f, 0.15f, 150.f, 160.f, 2, 3.f}; // hcmvs_set_geo_params (hcmvs_default_geo_params)
	bool haveGeoStats = false;            // the last estimate had an item with the geometric-consistency term active
	DevBuf dGeo{this};                    // GeoView [kMaxBatch][kMaxViews]
	std::vector<GeoView> hGeo;
	DevBuf sync{this};                    // int32_t: [0] unused, [1] error word, [16 .. 16 + kMaxBatch) row tickets of the batch items, then kMaxBatch rows-done counters
	SweepKnobs knobs;                     // the HCMVS_* tuning knobs of the environment (sweep_plan.h)
	DevBuf evals{this};                   // unsigned long long [16]: SweepSync::evals
	Event ev[4];                          // timing: before the init score, the sweeps, the end pass, and after it
	int lastSweeps = 0, lastSweepLaunches = 0;
	bool haveStats = false;
	int fuseOrder = 0; // hcmvs_set_fuse_order
	// filter / fuse scratch
	DevBuf dMaps{this};       // DevMap per view id
	DevBuf counters{this};    // unsigned long long [8]
	DevBuf fuseScratch{this};
	DevBuf filterStage{this}, filterTab{this}, filterCnt{this}; // hcmvs_filter_sequence: staging slabs, tables, per-image counters (its keys: fuseScratch)
	DevBuf passScratch{this}; // per-pass tables of the fusion (hcmvs_fuse_cloud, hcmvs_postfilter_sequence)
	DevBuf pfState;           // the post-filter chain's state kept from fusion to fusion (pf_kernels.hip); never reserved with the reclaimer
	bool errPending = false; // an estimate was enqueued since the error word was last read
	int nCU = 0;          // compute units of the device (sweep_plan.h)
	PinnedBuf pinned; // page-locked staging of the host-buffer uploads (a pageable hipMemcpy crawls at ~1.3 GB/s here), in two halves
	Event upEv[2] = {Event(hipEventDisableTiming), Event(hipEventDisableTiming)}; // a half has left for the device
	// hcmvs_*_init_device: the counters, the table and the tile lists of a call (init_plan.h InitLayout) on the device, and their page-locked
	// staging; initCopied marks the copy out of the staging, which is rewritten only after it
	DevBuf initBuf{this};
	PinnedBuf initPinned;
	Event initCopied{hipEventDisableTiming};
	bool initInFlight = false;
	Event initEv[2]; // timing: around the kernel
	hcmvs_init_stats initStats = {};
	bool haveInitStats = false;
	// hcmvs_handoff_maps_device: the result slots, the items and the prefix table of a call (handoff_plan.h HandoffLayout) on the device and
	// their page-locked staging, through which the slots also come back; the call synchronises, so nothing of it is in flight afterwards
	DevBuf handoffBuf{this};
	PinnedBuf handoffPinned;
	Event handoffEv[2]; // timing: around the kernels
	hcmvs_handoff_stats handoffStats = {};
	bool haveHandoffStats = false;
	// hcmvs_remove_speckles_batch_device: the result, the items, the tile table, the partials and the 8 B per pixel of a call
	// (speckle_plan.h SpeckleLayout) on the device, and the page-locked staging of the first three, through which the result also comes
	// back; the call synchronises, so nothing of it is in flight afterwards
	DevBuf speckleBuf{this};
	PinnedBuf specklePinned;
	Event speckleEv[2]; // timing: around the kernels
	// hcmvs_generate_plane_prior_device: the scratch of a call, kept for hcmvs_get_plane_prior_trace
	// (the reclaimer gives it back when memory is short: the trace is then gone, the next generate call allocates again)
	DevBuf priorGenKept{this};
	PriorGenTrace priorTrace;

	bool reclaim() override {
		if (!pfState.capacity() && !priorGenKept.capacity()) return false;
		(void)hipStreamSynchronize(stream);
		pfState.reset();
		priorGenKept.reset(); // the plane-prior scratch is only kept for hcmvs_get_plane_prior_trace
		priorTrace = PriorGenTrace();
		return true;
	}
};

static int fail(hcmvs_ctx* c, int code, const char* fmt, ...) {
	if (c) {
		char buf[512];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		c->err = buf;
	}
	return code;
}
#define HIPCHK(c, call)                                                                             \
	do {                                                                                            \
		hipError_t e_ = (call);                                                                     \
		if (e_ != hipSuccess) return fail(c, HCMVS_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
	} while (0)

// the registered view `id`, or null with the failure (HCMVS_ERR_INVALID) recorded for the entry point `who`
static View* find_view(hcmvs_ctx* c, const char* who, uint32_t id) {
	auto it = c->views.find(id);
	if (it != c->views.end()) return &it->second;
	fail(c, HCMVS_ERR_INVALID, "%s: unknown view %u", who, id);
	return nullptr;
}

#ifdef HCMVS_STAMPS
namespace hcmvs { void debug_read_stamps(unsigned long long* out, int reset); }
#endif
namespace hcmvs { // img_kernels.hip
void launch_resize_gray(const float* src, int sw, int sh, float* dst, int dw, int dh, float scaleParam, hipStream_t s);
void launch_ignore_mask(const uint16_t* labels, int lw, int lh, const int32_t* ignore, int nIgnore, uint8_t* keep, int W, int H, hipStream_t s);
}

extern "C" {

void hcmvs_default_params(hcmvs_params* p) {
	if (!p) return;
	memset(p, 0, sizeof *p);
	p->adapthalfwin = 5;           // DensifyPointCloud.cpp:163
	p->n_estimation_iters = 1;
	p->it_external = 0;
	p->n_external_iters = 1;
	p->propagate_halfwin = 1;
	p->propagate_step = 4;
	p->n_random_iters = 6;         // DepthMap.cpp:120
	p->ncc_threshold_keep = 0.55f; // DepthMap.cpp:117
	p->random_depth_ratio = 0.003f;
	p->random_angle1_deg = 16.f;
	p->random_angle2_deg = 10.f;
	p->random_smooth_depth = 0.02f;
	p->random_smooth_normal_deg = 13.f;
	p->random_smooth_bonus = 0.93f;
	p->photometric_flow = 0.f;
	p->seed = 1234;
	p->median_blur = 1;
}

int hcmvs_create(int device, hcmvs_ctx** out) {
	if (!out) return HCMVS_ERR_INVALID;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return HCMVS_ERR_NO_DEVICE;
	if (hipSetDevice(device) != hipSuccess) return HCMVS_ERR_NO_DEVICE;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HCMVS_ERR_NO_DEVICE;
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HCMVS_ERR_NO_DEVICE; // kernels are built for gfx950 only
	hcmvs_ctx* c = new hcmvs_ctx();
	c->device = device;
	c->nCU = prop.multiProcessorCount;
	if (hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) != hipSuccess) { hcmvs_destroy(c); return HCMVS_ERR_NO_DEVICE; }
	c->stream = c->ownStream;
	for (Event& e : c->ev)
		if (e.ensure() != hipSuccess) { hcmvs_destroy(c); return HCMVS_ERR_NO_DEVICE; }
	c->hViews.resize((size_t)kMaxBatch * kViewSlotEntries); c->hItems.resize(kMaxBatch); c->hSpread.resize((size_t)kMaxBatch * kMaxViews);
	c->hGeo.resize((size_t)kMaxBatch * kMaxViews);
	if (c->dViews.reserve(sizeof(DevView) * kViewSlotEntries * kMaxBatch, c->stream) != hipSuccess || c->evals.reserve(128, c->stream) != hipSuccess ||
	    c->dSpread.reserve(sizeof(SpreadView) * kMaxViews * kMaxBatch, c->stream) != hipSuccess ||
	    c->dGeo.reserve(sizeof(GeoView) * kMaxViews * kMaxBatch, c->stream) != hipSuccess ||
	    c->dItems.reserve(sizeof(EstConst) * kMaxBatch, c->stream) != hipSuccess || c->sync.reserve(64 + sizeof(int32_t) * 2 * kMaxBatch, c->stream) != hipSuccess) {
		hcmvs_destroy(c);
		return HCMVS_ERR_NO_DEVICE;
	}
	c->knobs = parse_sweep_knobs(getenv("HCMVS_SWEEP_LAG"), getenv("HCMVS_XCD_AFFINITY"), getenv("HCMVS_SWEEP_LAUNCHES"), getenv("HCMVS_SWEEP_SEGMENT"),
	                             getenv("HCMVS_WAVES_PER_ROW"));
	*out = c;
	return HCMVS_OK;
}

void hcmvs_destroy(hcmvs_ctx* c) {
	if (!c) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream); // the stream is idle: the device buffers go with the context
	const hipStream_t own = c->ownStream;
	delete c; // every buffer and event goes with its owner
	if (own) (void)hipStreamDestroy(own);
}

const char* hcmvs_last_error(const hcmvs_ctx* c) { return c ? c->err.c_str() : "null context"; }

// A sweep worker that gave up waiting on its predecessor row leaves the error word set (pm_kernels.hip wait_progress):
// every synchronising entry point reports it, so a caller of the asynchronous *_device entries learns of it without a
// separate hcmvs_get_stats.  The stream must be idle.
static int check_sweep_error(hcmvs_ctx* c) {
	if (!c->errPending) return HCMVS_OK;
	int32_t flags[2] = {0, 0};
	HIPCHK(c, hipMemcpy(flags, c->sync.get(), sizeof flags, hipMemcpyDeviceToHost));
	c->errPending = false;
	if (flags[1] != 0) return fail(c, HCMVS_ERR_TIMEOUT, "sweep worker timed out waiting for its predecessor row; the maps of the last estimate are incomplete");
	return HCMVS_OK;
}

int hcmvs_set_stream(hcmvs_ctx* c, void* stream) {
	if (!c) return HCMVS_ERR_INVALID;
	c->stream = stream ? (hipStream_t)stream : c->ownStream;
	return HCMVS_OK;
}
int hcmvs_synchronize(hcmvs_ctx* c) {
	if (!c) return HCMVS_ERR_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return check_sweep_error(c);
}

// host -> device through the context's page-locked staging buffer, in pieces: the caller's buffer is pageable, and a pageable
// hipMemcpy is an order of magnitude slower than memcpy + a pinned transfer
static int upload_staged(hcmvs_ctx* c, void* dst, const void* src, size_t bytes) {
	{ // a caller that already holds the data in page-locked memory (allocated by or registered with the runtime) needs no staging
		hipPointerAttribute_t at;
		if (hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost) {
			HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream));
			return HCMVS_OK;
		}
		(void)hipGetLastError(); // pageable memory is "invalid value" to the query
	}
	const size_t piece = (size_t)32 << 20;
	if (c->pinned.reserve(2 * piece) != hipSuccess) { // no pinned memory to be had: the plain copy
		HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		return HCMVS_OK;
	}
	for (Event& e : c->upEv) HIPCHK(c, e.ensure());
	const hipEvent_t done[2] = {c->upEv[0].get(), c->upEv[1].get()};
	bool used[2] = {false, false};
	int k = 0;
	for (size_t off = 0; off < bytes; off += piece, k ^= 1) {
		const size_t n = std::min(piece, bytes - off);
		if (used[k]) HIPCHK(c, hipEventSynchronize(done[k])); // the half I am about to overwrite has left
		memcpy(c->pinned.get() + (size_t)k * piece, (const char*)src + off, n);
		HIPCHK(c, hipMemcpyAsync((char*)dst + off, c->pinned.get() + (size_t)k * piece, n, hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipEventRecord(done[k], c->stream));
		used[k] = true;
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return HCMVS_OK;
}

static int set_view(hcmvs_ctx* c, uint32_t id, int w, int h, const float* gray, const uint8_t* bgr, const double* K,
                    const double* R, const double* C, bool copy) {
	if (!c) return HCMVS_ERR_INVALID;
	// gray may be null when a colour image is given: a view that is only fused / filtered (camera, colours, gradient map), never the
	// reference or a source view of an estimate -- what a rank of a multi-GPU job holds of the images other ranks estimate
	if ((!gray && !bgr) || !K || !R || !C || w < 2 * kHalfWindow + 2 || h < 2 * kHalfWindow + 2 || w > 32768 || h > 32768 || id >= kMaxViewId)
		return fail(c, HCMVS_ERR_INVALID, "upload_view: bad arguments (id %u, %dx%d)", id, w, h);
	HIPCHK(c, hipSetDevice(c->device));
	auto it = c->views.find(id);
	if (it != c->views.end()) { HIPCHK(c, hipStreamSynchronize(c->stream)); it->second = View(c); } // the old buffers go before the new ones come
	View v(c);
	v.w = w; v.h = h;
	const size_t n = (size_t)w * h;
	if (copy) {
		if (gray) {
			HIPCHK(c, v.grayMem.reserve(n * sizeof(float), c->stream));
			v.gray = v.grayMem.get<float>();
			const int rc = upload_staged(c, v.gray, gray, n * sizeof(float));
			if (rc) return rc;
		}
		if (bgr) {
			HIPCHK(c, v.bgrMem.reserve(n * 3, c->stream));
			v.bgr = v.bgrMem.get<uint8_t>();
			const int rc = upload_staged(c, v.bgr, bgr, n * 3);
			if (rc) return rc;
		} // (upload_staged has synchronised: the caller may free its host buffers on return)
	} else {
		v.gray = const_cast<float*>(gray);
		v.bgr = const_cast<uint8_t*>(bgr);
	}
	memcpy(v.K, K, sizeof v.K); memcpy(v.R, R, sizeof v.R); memcpy(v.C, C, sizeof v.C);
	c->views[id] = std::move(v);
	return HCMVS_OK;
}

int hcmvs_upload_view(hcmvs_ctx* c, uint32_t id, int32_t w, int32_t h, const float* gray, const uint8_t* bgr,
                      const double K[9], const double R[9], const double C[3]) {
	return set_view(c, id, w, h, gray, bgr, K, R, C, true);
}
int hcmvs_set_view_device(hcmvs_ctx* c, uint32_t id, int32_t w, int32_t h, const float* gray, const uint8_t* bgr,
                          const double K[9], const double R[9], const double C[3]) {
	return set_view(c, id, w, h, gray, bgr, K, R, C, false);
}
int hcmvs_rescale_view(hcmvs_ctx* c, uint32_t src_id, uint32_t dst_id, float scale) {
	if (!c) return HCMVS_ERR_INVALID;
	auto it = c->views.find(src_id);
	if (it == c->views.end() || dst_id >= kMaxViewId || dst_id == src_id) return fail(c, HCMVS_ERR_INVALID, "rescale_view: bad view ids %u -> %u", src_id, dst_id);
	if (!(scale > 0.f) || fabsf(scale - 1.f) < 0.15f) return fail(c, HCMVS_ERR_INVALID, "rescale_view: scale %g is within 15 %% of 1 (DepthMap.h:234: not resampled)", scale);
	const View& src = it->second;
	if (!src.gray) return fail(c, HCMVS_ERR_INVALID, "rescale_view: view %u has no gray image (fuse-only view)", src_id);
	// cv::resize with dsize empty: Size(saturate_cast<int>(w * fx), saturate_cast<int>(h * fy)), saturate_cast<int>(double) = cvRound
	const int nw = (int)lrint((double)src.w * (double)scale), nh = (int)lrint((double)src.h * (double)scale);
	if (nw < 2 * kHalfWindow + 2 || nh < 2 * kHalfWindow + 2 || nw > 32768 || nh > 32768) return fail(c, HCMVS_ERR_INVALID, "rescale_view: %dx%d x %g gives an unusable size", src.w, src.h, scale);
	HIPCHK(c, hipSetDevice(c->device));
	auto old = c->views.find(dst_id);
	if (old != c->views.end()) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->views.erase(old); }
	View v(c);
	v.w = nw; v.h = nh;
	HIPCHK(c, v.grayMem.reserve((size_t)nw * nh * sizeof(float), c->stream));
	v.gray = v.grayMem.get<float>();
	hcmvs::launch_resize_gray(src.gray, src.w, src.h, v.gray, nw, nh, scale, c->stream);
	HIPCHK(c, hipGetLastError());
	// Image::GetCamera(platforms, size): K normalised by max(w, h) of the image, scaled to max(w', h') (Camera.h:167-180)
	const double f = (double)std::max(nw, nh) / (double)std::max(src.w, src.h);
	memcpy(v.K, src.K, sizeof v.K); memcpy(v.R, src.R, sizeof v.R); memcpy(v.C, src.C, sizeof v.C);
	v.K[0] *= f; v.K[4] *= f; v.K[2] *= f; v.K[5] *= f;
	v.rescaled = true;
	c->views[dst_id] = std::move(v);
	return HCMVS_OK;
}
int hcmvs_get_view_info(hcmvs_ctx* c, uint32_t id, int32_t* w, int32_t* h, double K[9]) {
	if (!c) return HCMVS_ERR_INVALID;
	const View* v = find_view(c, "get_view_info", id);
	if (!v) return HCMVS_ERR_INVALID;
	if (w) *w = v->w;
	if (h) *h = v->h;
	if (K) memcpy(K, v->K, sizeof(double) * 9);
	return HCMVS_OK;
}
int hcmvs_get_view_gray(hcmvs_ctx* c, uint32_t id, float* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	const View* v = find_view(c, "get_view_gray", id);
	if (!v) return HCMVS_ERR_INVALID;
	if (!v->gray) return fail(c, HCMVS_ERR_INVALID, "get_view_gray: view %u was registered without a gray image (fuse-only view)", id);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(out, v->gray, (size_t)v->w * v->h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return HCMVS_OK;
}

int hcmvs_release_view(hcmvs_ctx* c, uint32_t id) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!find_view(c, "release_view", id)) return HCMVS_ERR_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->views.erase(id);
	return HCMVS_OK;
}

static int ensure_slot(hcmvs_ctx* c, int i, size_t n, int rows) {
	while ((int)c->slots.size() <= i) c->slots.emplace_back(c);
	hcmvs_ctx::Slot& sl = c->slots[i];
	HIPCHK(c, sl.dn.reserve(n * sizeof(float4), c->stream));
	HIPCHK(c, sl.conf.reserve(n * sizeof(float), c->stream));
	HIPCHK(c, sl.tmpDepth.reserve(n * sizeof(float), c->stream));
	HIPCHK(c, sl.progress.reserve((size_t)rows * kProgressStride * sizeof(int32_t), c->stream));
	return HCMVS_OK;
}

// SceneDensify.cpp:581-595 InitGraMap, computed once per view on the device
static int ensure_gradient(hcmvs_ctx* c, View& v) {
	if (v.gra.capacity()) return HCMVS_OK;
	const int n = v.w * v.h;
	HIPCHK(c, c->tmpU8.reserve((size_t)n, c->stream));
	HIPCHK(c, v.gra.reserve((size_t)n, c->stream));
	if (v.bgr) launch_bgr_to_u8(v.bgr, c->tmpU8.get<uint8_t>(), n, c->stream);
	else launch_gray_to_u8(v.gray, c->tmpU8.get<uint8_t>(), n, c->stream);
	launch_gradient_map(c->tmpU8.get<uint8_t>(), v.gra.get<uint8_t>(), v.w, v.h, c->stream);
	HIPCHK(c, hipGetLastError());
	return HCMVS_OK;
}

// the layout the scorer samples a source view from (pm_kernels.hip quad_kernel), built once per view
static int ensure_quads(hcmvs_ctx* c, View& v) {
	if (v.quads.capacity()) return HCMVS_OK;
	HIPCHK(c, v.quads.reserve((size_t)v.w * v.h * sizeof(float4), c->stream));
	launch_quads(v.gray, v.quads.get<float4>(), v.w, v.h, c->stream);
	HIPCHK(c, hipGetLastError());
	return HCMVS_OK;
}

int hcmvs_get_gradient_map(hcmvs_ctx* c, uint32_t id, uint8_t* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	View* v = find_view(c, "get_gradient_map", id);
	if (!v) return HCMVS_ERR_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = ensure_gradient(c, *v);
	if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(out, v->gra.get(), (size_t)v->w * v->h, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return HCMVS_OK;
}

// --ignore-mask-label (DepthEstimator::ImportIgnoreMask, DepthMap.cpp:319-348): the keep-mask of view `id` as a reference view, from a
// 16-bit label image of any size, on the host or (device) in device memory.  labels == null removes the mask.
static int set_ignore_mask(hcmvs_ctx* c, uint32_t id, const uint16_t* labels, int32_t lw, int32_t lh, const int32_t* ignore, int32_t nIgnore,
                           bool device) {
	if (!c) return HCMVS_ERR_INVALID;
	View* pv = find_view(c, "set_ignore_mask", id);
	if (!pv) return HCMVS_ERR_INVALID;
	View& v = *pv;
	HIPCHK(c, hipSetDevice(c->device));
	if (!labels) { // (an estimate in flight may still read the old mask)
		HIPCHK(c, hipStreamSynchronize(c->stream));
		v.keep.reset();
		return HCMVS_OK;
	}
	if (lw < 1 || lh < 1 || lw > 65536 || lh > 65536 || nIgnore < 0 || (nIgnore > 0 && !ignore))
		return fail(c, HCMVS_ERR_INVALID, "set_ignore_mask: bad arguments (view %u, label image %dx%d, %d labels)", id, lw, lh, nIgnore);
	// mask(r,c) == atoi(label) compares a 16-bit value with an int: labels outside 0 .. 65535 never match
	std::vector<int32_t> lab;
	for (int i = 0; i < nIgnore; ++i)
		if (ignore[i] >= 0 && ignore[i] <= 65535 && std::find(lab.begin(), lab.end(), ignore[i]) == lab.end()) lab.push_back(ignore[i]);
	const size_t imgBytes = (size_t)lw * lh * sizeof(uint16_t);
	Carve cv;
	const size_t oImg = device ? 0 : cv(imgBytes), oLab = cv(sizeof(int32_t) * (lab.size() + 1));
	HIPCHK(c, c->maskStage.reserve(cv.size, c->stream));
	HIPCHK(c, v.keep.reserve((size_t)v.w * v.h, c->stream));
	const uint16_t* dLabels = labels;
	if (!device) {
		const int rc = upload_staged(c, c->maskStage.get() + oImg, labels, imgBytes);
		if (rc) return rc;
		dLabels = (const uint16_t*)(c->maskStage.get() + oImg);
	}
	int32_t* dIgnore = (int32_t*)(c->maskStage.get() + oLab);
	if (!lab.empty()) HIPCHK(c, hipMemcpyAsync(dIgnore, lab.data(), sizeof(int32_t) * lab.size(), hipMemcpyHostToDevice, c->stream));
	launch_ignore_mask(dLabels, lw, lh, dIgnore, (int)lab.size(), v.keep.get<uint8_t>(), v.w, v.h, c->stream);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (lab and the staging go on being used by the next call)
	return HCMVS_OK;
}

int hcmvs_set_ignore_mask(hcmvs_ctx* c, uint32_t id, const uint16_t* labels, int32_t lw, int32_t lh, const int32_t* ignore, int32_t n_ignore) {
	return set_ignore_mask(c, id, labels, lw, lh, ignore, n_ignore, false);
}
int hcmvs_set_ignore_mask_device(hcmvs_ctx* c, uint32_t id, const uint16_t* d_labels, int32_t lw, int32_t lh, const int32_t* ignore,
                                 int32_t n_ignore) {
	return set_ignore_mask(c, id, d_labels, lw, lh, ignore, n_ignore, true);
}
int hcmvs_get_ignore_mask(hcmvs_ctx* c, uint32_t id, uint8_t* keep) {
	if (!c || !keep) return HCMVS_ERR_INVALID;
	const View* pv = find_view(c, "get_ignore_mask", id);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	if (!v.keep.capacity()) { memset(keep, 1, (size_t)v.w * v.h); return HCMVS_OK; } // no mask: every pixel is estimated
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(keep, v.keep.get(), (size_t)v.w * v.h, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return HCMVS_OK;
}

// an estimate call the plan refuses (est_plan.h), in the words of the API.  ref: the reference view of item bad.at (kEstBorder)
static int refuse_estimate(hcmvs_ctx* c, EstCheck bad, const hcmvs_batch_item* items, int n_items, const hcmvs_params* p, const View* ref = nullptr) {
	switch (bad.broken) {
	case kEstOk: return HCMVS_OK;
	case kEstBatchSize: return fail(c, HCMVS_ERR_INVALID, "estimate: batch size %d not in 1..%d", n_items, kMaxBatch);
	case kEstHalfWindow: return fail(c, HCMVS_ERR_INVALID, "estimate: adapthalfwin %d not in 1..%d", p->adapthalfwin, kMaxHalfWindow);
	case kEstIterCounts: return fail(c, HCMVS_ERR_INVALID, "estimate: bad iteration counts");
	case kEstSrcCount: // (a count outside 1..16 is of neither class)
	case kEstSrcClass: return fail(c, HCMVS_ERR_INVALID, "estimate: the items of a batch must use source-view counts of one class (1-8 or 9-16)");
	case kEstNull: return fail(c, HCMVS_ERR_INVALID, "estimate: null argument");
	case kEstDepthRange: return fail(c, HCMVS_ERR_INVALID, "estimate: bad depth range [%g,%g)", items[bad.at].d_min, items[bad.at].d_max);
	case kEstBorder:
		return fail(c, HCMVS_ERR_INVALID, "estimate: view %u (%dx%d) has no pixel inside the %d px border", items[bad.at].ref_id, ref->w, ref->h, est_border(*p));
	case kEstPriorHint:
		return fail(c, HCMVS_ERR_INVALID, "estimate: item %d (view %u) offers the `restore` hint in its last outer iteration while an item of the batch has an "
		            "active depth prior: the prior term is not combined with the hint (remove one of the two)", bad.at, items[bad.at].ref_id);
	case kEstPriorSpread:
		return fail(c, HCMVS_ERR_INVALID, "estimate: view spread has maps to try for item %d (view %u) while an item of the batch has an active depth prior: "
		            "the prior term is not combined with view spread (hcmvs_set_viewspread(ctx, 0), as the reference's schedule runs priors)", bad.at, items[bad.at].ref_id);
	case kEstSweepRange:
		return fail(c, HCMVS_ERR_INVALID, "estimate_sweeps: first_sweep >= 0, n_sweeps >= 1 and a last index <= %d are needed (the random stream of a sweep "
		            "is it_external * 64 + 1 + index)", HCMVS_MAX_SWEEP_INDEX);
	case kEstGeoHint:
		return fail(c, HCMVS_ERR_INVALID, "estimate: item %d (view %u) offers the `restore` hint in its last outer iteration while the geometric-consistency "
		            "term is active for an item of the batch: the term is not combined with the hint (remove one of the two)", bad.at, items[bad.at].ref_id);
	case kEstGeoSpread:
		return fail(c, HCMVS_ERR_INVALID, "estimate: view spread has maps to try for item %d (view %u) while the geometric-consistency term is active for an "
		            "item of the batch: the term is not combined with view spread (hcmvs_set_viewspread(ctx, 0))", bad.at, items[bad.at].ref_id);
	case kEstGeoPrior:
		return fail(c, HCMVS_ERR_INVALID, "estimate: item %d (view %u) has an active depth prior while the geometric-consistency term is active for an item of "
		            "the batch: the two terms are not combined (remove the prior, or switch the term off)", bad.at, items[bad.at].ref_id);
	}
	return HCMVS_ERR_INVALID;
}

static EstCamera camera_of(const View& v) { return {v.K, v.R, v.C, v.w, v.h}; }

// Item `slot` of a batch into hItems / hViews / hSpread: the plan's constants (est_plan.h) and what only the context knows -- the views'
// device images, made when first needed, the slot's working maps and the caller's pointers
static int build_item(hcmvs_ctx* c, int slot, const hcmvs_batch_item* items, int n_items, const hcmvs_params* p, bool sweepsOnly, int firstSweep) {
	const hcmvs_batch_item& it = items[slot];
	int rc = refuse_estimate(c, est_check_item(items, slot), items, n_items, p);
	if (rc) return rc;
	const int n_src = it.n_src;
	View* pref = find_view(c, "estimate", it.ref_id);
	if (!pref) return HCMVS_ERR_INVALID;
	View& ref = *pref;
	if (!ref.gray) return fail(c, HCMVS_ERR_INVALID, "estimate: view %u was registered without a gray image (fuse-only view)", it.ref_id);
	rc = refuse_estimate(c, est_check_image(slot, ref.w, ref.h, *p), items, n_items, p, &ref);
	if (rc) return rc;
	const bool priorActive = est_prior_active(ref.prior != nullptr, c->prior, *p);
	rc = ensure_slot(c, slot, (size_t)ref.w * ref.h, ref.h);
	if (rc) return rc;
	rc = ensure_gradient(c, ref);
	if (rc) return rc;
	const View* src[kMaxViews]; // the source views, looked up once
	EstCamera cam[kMaxViews];
	uint64_t imgAt[kMaxViews];
	size_t imgBytes[kMaxViews];
	for (int v = 0; v < n_src; ++v) {
		View* s = find_view(c, "estimate", it.src_ids[v]);
		if (!s) return HCMVS_ERR_INVALID;
		if (!s->gray) return fail(c, HCMVS_ERR_INVALID, "estimate: source view %u was registered without a gray image (fuse-only view)", it.src_ids[v]);
		rc = ensure_quads(c, *s);
		if (rc) return rc;
		src[v] = s; cam[v] = camera_of(*s);
		imgAt[v] = (uintptr_t)s->quads.get(); imgBytes[v] = (size_t)s->w * s->h * sizeof(float4);
	}
	EstConst& k = c->hItems[slot];
	DevView* hv = c->hViews.data() + (size_t)slot * kViewSlotEntries;
	const bool hint = !sweepsOnly && it.d_hint_depth && it.d_hint_normal; // (the sweeps-only entry never offers the hint)
	est_item_consts(camera_of(ref), cam, n_src, *p, it.d_min, it.d_max, it.seed_offset, hint, k, hv);
	k.ref = ref.gray; k.gra = ref.gra.get<uint8_t>(); k.views = c->dViews.get<DevView>() + (size_t)slot * kViewSlotEntries;
	uint32_t imgOff[kMaxViews];
	const EstWindow win = est_image_window(imgAt, imgBytes, n_src, imgOff);
	if (win.kind == kEstWindowRefused) return fail(c, HCMVS_ERR_INVALID, "estimate: the source images of one item exceed 4 GiB");
	for (int v = 0; v < n_src; ++v) hv[v].byteOff = imgOff[v];
	if (win.kind == kEstWindowDirect) k.imgBase = (const char*)(uintptr_t)win.base;
	else { // the caller's images lie further apart: copied (device to device, a few tens of MB) into a compact slab owned by the context
		DevBuf& srcSlab = c->slots[slot].srcSlab;
		HIPCHK(c, srcSlab.reserve(win.slabBytes, c->stream));
		for (int v = 0; v < n_src; ++v)
			HIPCHK(c, hipMemcpyAsync(srcSlab.get() + imgOff[v], src[v]->quads.get(), imgBytes[v], hipMemcpyDeviceToDevice, c->stream));
		k.imgBase = srcSlab.get();
	}
	k.dn = c->slots[slot].dn.get<float4>(); k.conf = c->slots[slot].conf.get<float>(); k.progress = c->slots[slot].progress.get<int32_t>();
	if (est_uses_hint(*p, hint)) { k.hintDepth = it.d_hint_depth; k.hintNormal = it.d_hint_normal; }
	k.keep = ref.keep.capacity() ? ref.keep.get<uint8_t>() : nullptr; // the reference view's mask only (source views ignore theirs)
	SpreadView* hs = c->hSpread.data() + (size_t)slot * kMaxViews;
	memset(hs, 0, sizeof(SpreadView) * kMaxViews);
	for (int v = 0; v < n_src; ++v) {
		const View& s = *src[v];
		if (!est_view_spreads(c->viewspread, *p, s.sDepth, s.rescaled)) continue;
		hs[v].depth = s.sDepth; hs[v].normal = s.sNormal; hs[v].conf = s.sConf;
		est_spread_consts(camera_of(ref), cam[v], hs[v]);
		k.spread = c->dSpread.get<SpreadView>() + (size_t)slot * kMaxViews;
	}
	PriorItem& pi = *prior_item(hv); // behind the item's views
	memset(&pi, 0, sizeof pi);
	if (priorActive) {
		pi.prior = ref.prior;
		est_prior_consts(c->prior, sweepsOnly ? firstSweep : -1, pi); // (no init-score pass: the call's first sweep counts the pixels with a usable prior)
	}
	GeoItem& gi = *geo_item(hv); // behind the PriorItem
	memset(&gi, 0, sizeof gi);
	GeoView* hg = c->hGeo.data() + (size_t)slot * kMaxViews;
	memset(hg, 0, sizeof(GeoView) * kMaxViews);
	bool offers = false;
	for (int v = 0; v < n_src; ++v) offers = offers || est_geo_offers(src[v]->sDepth != nullptr, src[v]->rescaled);
	if (est_geo_active(c->geo, *p, offers)) {
		for (int v = 0; v < n_src; ++v) {
			const View& s = *src[v];
			est_geo_view(camera_of(ref), cam[v], hg[v]);
			if (est_geo_offers(s.sDepth != nullptr, s.rescaled)) { hg[v].depth = s.sDepth; hg[v].normal = s.sNormal; }
		}
		gi.views = c->dGeo.get<GeoView>() + (size_t)slot * kMaxViews;
		est_geo_consts(c->geo, sweepsOnly ? firstSweep : -1, gi);
	}
	return HCMVS_OK;
}

// hcmvs_estimate_batch_device (sweepsOnly false: [mask] -> [median] -> init score -> n_estimation_iters sweeps -> end pass) and
// hcmvs_estimate_sweeps_batch_device (sweepsOnly: import of depth, normal and conf -> sweeps firstSweep .. firstSweep + nSweeps - 1 -> end pass)
static int estimate_batch(hcmvs_ctx* c, const hcmvs_batch_item* items, int32_t n_items, const hcmvs_params* p, bool sweepsOnly, int firstSweep, int nSweeps) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!items || !p) return fail(c, HCMVS_ERR_INVALID, "estimate: null argument");
	int rc = refuse_estimate(c, est_check_call(n_items, *p), items, n_items, p);
	if (rc) return rc;
	if (sweepsOnly) {
		rc = refuse_estimate(c, est_check_sweeps(firstSweep, nSweeps), items, n_items, p);
		if (rc) return rc;
	}
	{ // An active prior anywhere in the batch is refused together with a hint in effect or with view spread at work, before anything
	  // reaches the device.  (Items that name unknown views are refused by build_item, in item order, as before.)
		std::vector<char> flags(3 * (size_t)n_items, 0);
		bool* priorActive = (bool*)flags.data(); bool* hintInEffect = priorActive + n_items; bool* spreadWork = hintInEffect + n_items;
		for (int i = 0; i < n_items; ++i) {
			const hcmvs_batch_item& it = items[i];
			auto rv = c->views.find(it.ref_id);
			priorActive[i] = rv != c->views.end() && est_prior_active(rv->second.prior != nullptr, c->prior, *p);
			hintInEffect[i] = !sweepsOnly && est_uses_hint(*p, it.d_hint_depth && it.d_hint_normal);
			for (int v = 0; it.src_ids && v < it.n_src && v < kMaxViews; ++v) {
				auto sv = c->views.find(it.src_ids[v]);
				if (sv != c->views.end() && est_view_spreads(c->viewspread, *p, sv->second.sDepth, sv->second.rescaled)) spreadWork[i] = true;
			}
		}
		rc = refuse_estimate(c, est_check_prior_batch(priorActive, hintInEffect, spreadWork, n_items), items, n_items, p);
		if (rc) return rc;
		// the geometric-consistency term active anywhere in the batch: refused together with a hint, view spread at work or an active prior
		std::vector<char> gflags((size_t)n_items, 0);
		bool* geoActive = (bool*)gflags.data();
		for (int i = 0; i < n_items; ++i) {
			const hcmvs_batch_item& it = items[i];
			bool offers = false;
			for (int v = 0; it.src_ids && v < it.n_src && v < kMaxViews; ++v) {
				auto sv = c->views.find(it.src_ids[v]);
				if (sv != c->views.end() && est_geo_offers(sv->second.sDepth != nullptr, sv->second.rescaled)) offers = true;
			}
			geoActive[i] = est_geo_active(c->geo, *p, offers);
		}
		rc = refuse_estimate(c, est_check_geo_batch(geoActive, hintInEffect, spreadWork, priorActive, n_items), items, n_items, p);
		if (rc) return rc;
	}
	HIPCHK(c, hipSetDevice(c->device));
	int maxRows = 0;
	bool spread = false, prior = false, geo = false;
	hcmvs::SweepBatch batch;
	batch.big = p->adapthalfwin > kHalfWindow; batch.nSweeps = nSweeps; batch.firstSweep = firstSweep; batch.nCU = c->nCU;
	batch.sweepPerLaunch = c->knobs.perLaunch; batch.sweepSegment = c->knobs.segment; batch.wavesPerRow = c->knobs.wavesPerRow;
	batch.items.reserve(n_items);
	for (int i = 0; i < n_items; ++i) {
		rc = build_item(c, i, items, n_items, p, sweepsOnly, firstSweep);
		if (rc) return rc;
		const EstConst& k = c->hItems[i];
		const bool itemPrior = prior_item(c->hViews.data() + (size_t)i * kViewSlotEntries)->prior != nullptr;
		const bool itemGeo = geo_item(c->hViews.data() + (size_t)i * kViewSlotEntries)->views != nullptr;
		batch.items.push_back(est_sweep_item(k, batch.nSweeps, itemPrior, itemGeo));
		maxRows = std::max(maxRows, batch.items.back().rows);
		spread = spread || k.spread;
		prior = prior || itemPrior;
		geo = geo || itemGeo;
	}
	if (spread) { // a launch must not read what it writes
		const EstOverlap o = est_spread_overlap(c->hItems.data(), c->hSpread.data(), items, n_items);
		if (o.item >= 0)
			return fail(c, HCMVS_ERR_INVALID, "estimate: the in/out maps of item %d (view %u) overlap the spread maps of source view %u of item %d: "
			            "a launch must not read what it writes (register a copy, or estimate the two images in separate calls)", o.item, items[o.item].ref_id,
			            items[o.other].src_ids[o.view], o.other);
	}
	if (geo) { // the same rule for the maps the geometric-consistency term reads
		std::vector<char> act((size_t)n_items, 0);
		for (int i = 0; i < n_items; ++i) act[i] = batch.items[i].geo;
		const EstOverlap o = est_geo_overlap(c->hItems.data(), c->hGeo.data(), (const bool*)act.data(), items, n_items);
		if (o.item >= 0)
			return fail(c, HCMVS_ERR_INVALID, "estimate: the in/out maps of item %d (view %u) overlap the maps source view %u of item %d offers to the "
			            "geometric-consistency term: a launch must not read what it writes (register a copy, or estimate the two images in separate calls)",
			            o.item, items[o.item].ref_id, items[o.other].src_ids[o.view], o.other);
	}
	hipStream_t s = c->stream;
	// same stream => the previous call's kernels are done with these tables before the copies land
	if (geo) HIPCHK(c, hipMemcpyAsync(c->dGeo.get(), c->hGeo.data(), sizeof(GeoView) * kMaxViews * n_items, hipMemcpyHostToDevice, s));
	c->haveGeoStats = geo;
	if (spread) HIPCHK(c, hipMemcpyAsync(c->dSpread.get(), c->hSpread.data(), sizeof(SpreadView) * kMaxViews * n_items, hipMemcpyHostToDevice, s));
	c->haveSpreadStats = spread;
	c->havePriorStats = prior;
	HIPCHK(c, hipMemcpyAsync(c->dViews.get(), c->hViews.data(), sizeof(DevView) * kViewSlotEntries * n_items, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemcpyAsync(c->dItems.get(), c->hItems.data(), sizeof(EstConst) * n_items, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemsetAsync(c->evals.get(), 0, 128, s));
	HIPCHK(c, hipMemsetAsync(c->sync.get(), 0, 64 + sizeof(int32_t) * 2 * kMaxBatch, s));

	HIPCHK(c, hipEventRecord(c->ev[0].get(), s));
	for (int i = 0; i < n_items; ++i) {
		const EstConst& k = c->hItems[i];
		if (sweepsOnly) { launch_import_state(k, items[i].d_depth, items[i].d_normal, items[i].d_conf, s); continue; }
		const float* depthIn = items[i].d_depth;
		// ApplyIgnoreMask on the initial maps, then the median (SceneDensify.cpp:776-860): an ignored pixel may come out of the median
		// with a positive depth (five or more valid neighbours) -- kept, with its zero normal, as the reference does
		if (k.keep) launch_apply_mask(k.keep, items[i].d_depth, items[i].d_normal, k.W * k.H, s);
		if (p->median_blur) { // SceneDensify.cpp:859
			launch_median3(items[i].d_depth, c->slots[i].tmpDepth.get<float>(), k.W, k.H, s);
			depthIn = c->slots[i].tmpDepth.get<float>();
		}
		launch_score_pass(k, depthIn, items[i].d_normal, c->evals.get<unsigned long long>(), s, batch.items[i].prior, batch.items[i].geo);
	}
	HIPCHK(c, hipEventRecord(c->ev[1].get(), s));
	int32_t* sync = c->sync.get<int32_t>();
	const SweepArgs sa{c->dItems.get<EstConst>(), n_items, maxRows, {sync + 16, sync + 16 + kMaxBatch, sync + 1, c->evals.get<unsigned long long>()}, c->knobs.lag, c->knobs.affinity};
	const std::vector<hcmvs::SweepLaunch> plan = hcmvs::plan_sweeps(batch); // HCMVS_SWEEP_LAUNCHES, HCMVS_SWEEP_SEGMENT, HCMVS_WAVES_PER_ROW
	for (const hcmvs::SweepLaunch& l : plan) {
		HIPCHK(c, hipMemsetAsync(sync + 16, 0, sizeof(int32_t) * 2 * kMaxBatch, s)); // tickets + rowsDone; the error word stays sticky
		for (int i = 0; i < n_items; ++i)
			HIPCHK(c, hipMemsetAsync(c->slots[i].progress.get(), 0, (size_t)batch.items[i].rows * kProgressStride * sizeof(int32_t), s));
		if (!launch_sweep(sa, l, s))
			return fail(c, HCMVS_ERR_INVALID, "estimate: no sweep kernel for %d waves per row, big %d two %d pack %d hint %d mask %d spread %d prior %d geo %d",
			            l.v.nw, l.v.big, l.v.two, l.v.pack, l.v.hint, l.v.mask, l.v.spread, l.v.prior, l.v.geo);
	}
	c->lastSweepLaunches = (int)plan.size();
	HIPCHK(c, hipEventRecord(c->ev[2].get(), s));
	for (int i = 0; i < n_items; ++i)
		launch_end_pass(c->hItems[i], p->it_external == p->n_external_iters - 1 ? 1 : 0, items[i].d_depth, items[i].d_normal, items[i].d_conf, s);
	HIPCHK(c, hipEventRecord(c->ev[3].get(), s));
	HIPCHK(c, hipGetLastError());
	c->lastSweeps = nSweeps;
	c->haveStats = true;
	c->errPending = true;
	return HCMVS_OK;
}

int hcmvs_estimate_batch_device(hcmvs_ctx* c, const hcmvs_batch_item* items, int32_t n_items, const hcmvs_params* p) {
	return estimate_batch(c, items, n_items, p, false, 0, p ? p->n_estimation_iters : 0);
}
int hcmvs_estimate_sweeps_batch_device(hcmvs_ctx* c, const hcmvs_batch_item* items, int32_t n_items, const hcmvs_params* p, int32_t first_sweep,
                                       int32_t n_sweeps) {
	return estimate_batch(c, items, n_items, p, true, first_sweep, n_sweeps);
}

int hcmvs_estimate_device(hcmvs_ctx* c, uint32_t ref_id, const uint32_t* src_ids, int32_t n_src, const hcmvs_params* p,
                          float d_min, float d_max, float* d_depth, float* d_normal, float* d_conf) {
	hcmvs_batch_item it;
	memset(&it, 0, sizeof it);
	it.ref_id = ref_id; it.src_ids = src_ids; it.n_src = n_src; it.d_min = d_min; it.d_max = d_max;
	it.d_depth = d_depth; it.d_normal = d_normal; it.d_conf = d_conf; it.seed_offset = 0;
	return hcmvs_estimate_batch_device(c, &it, 1, p);
}

int hcmvs_get_stats(hcmvs_ctx* c, hcmvs_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	memset(out, 0, sizeof *out);
	if (!c->haveStats) return fail(c, HCMVS_ERR_INVALID, "get_stats: no estimate has run");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	unsigned long long ev[4] = {0, 0, 0, 0};
	HIPCHK(c, hipMemcpy(ev, c->evals.get(), 32, hipMemcpyDeviceToHost));
	out->evals = ev[0];
	out->evals_issued = ev[1];
	out->tap_evals = ev[2];
	HIPCHK(c, hipEventElapsedTime(&out->ms_score, c->ev[0].get(), c->ev[1].get()));
	HIPCHK(c, hipEventElapsedTime(&out->ms_sweeps, c->ev[1].get(), c->ev[2].get()));
	HIPCHK(c, hipEventElapsedTime(&out->ms_end, c->ev[2].get(), c->ev[3].get()));
	HIPCHK(c, hipEventElapsedTime(&out->ms_total, c->ev[0].get(), c->ev[3].get()));
	out->n_sweeps = c->lastSweeps;
	out->n_sweep_launches = c->lastSweepLaunches;
	out->ms_sweep_avg = c->lastSweeps > 0 ? out->ms_sweeps / (float)c->lastSweeps : 0.f;
	c->errPending = true;
	return check_sweep_error(c);
}

// ---- depth priors (DepthMap.cpp:941-954) ----

void hcmvs_default_prior_params(hcmvs_prior_params* p) {
	if (!p) return;
	p->para_prior = 0.5f; p->sigma_prior = 0.2f; p->photo2geo = 2; // DensifyPointCloud.cpp:162, :175, :183
}
int hcmvs_set_prior_params(hcmvs_ctx* c, const hcmvs_prior_params* p) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!p) return fail(c, HCMVS_ERR_INVALID, "set_prior_params: null argument");
	switch (est_check_prior_params(*p)) {
	case kPriorOk: break;
	case kPriorPara: return fail(c, HCMVS_ERR_INVALID, "set_prior_params: para_prior %g is not in [0, 1]", (double)p->para_prior);
	case kPriorSigma: return fail(c, HCMVS_ERR_INVALID, "set_prior_params: sigma_prior %g is not a finite number > 0", (double)p->sigma_prior);
	case kPriorPhoto2geo: return fail(c, HCMVS_ERR_INVALID, "set_prior_params: photo2geo %d is negative", p->photo2geo);
	}
	c->prior = *p;
	return HCMVS_OK;
}
static int set_depth_prior(hcmvs_ctx* c, uint32_t id, const float* prior, bool copy) {
	if (!c) return HCMVS_ERR_INVALID;
	View* pv = find_view(c, "set_depth_prior", id);
	if (!pv) return HCMVS_ERR_INVALID;
	View& v = *pv;
	HIPCHK(c, hipSetDevice(c->device));
	if (!prior) { // (an estimate in flight may still read the old prior)
		HIPCHK(c, hipStreamSynchronize(c->stream));
		v.prior = nullptr;
		v.priorMem.reset();
		return HCMVS_OK;
	}
	if (v.rescaled) return fail(c, HCMVS_ERR_INVALID, "set_depth_prior: view %u was made by hcmvs_rescale_view: only a reference view's prior is ever read", id);
	if (!copy) { v.prior = prior; v.priorMem.reset(); return HCMVS_OK; }
	const size_t bytes = (size_t)v.w * v.h * sizeof(float);
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (an estimate in flight may still read the copy that is about to be overwritten)
	HIPCHK(c, v.priorMem.reserve(bytes, c->stream));
	const int rc = upload_staged(c, v.priorMem.get(), prior, bytes);
	if (rc) return rc;
	v.prior = v.priorMem.get<float>();
	return HCMVS_OK;
}
int hcmvs_set_depth_prior_device(hcmvs_ctx* c, uint32_t id, const float* d_prior) { return set_depth_prior(c, id, d_prior, false); }
int hcmvs_set_depth_prior(hcmvs_ctx* c, uint32_t id, const float* prior) { return set_depth_prior(c, id, prior, true); }
int hcmvs_get_prior_stats(hcmvs_ctx* c, hcmvs_prior_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	memset(out, 0, sizeof *out);
	if (!c->haveStats) return fail(c, HCMVS_ERR_INVALID, "get_prior_stats: no estimate has run");
	if (!c->havePriorStats) return HCMVS_OK; // the last estimate had no active prior: all zero
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	unsigned long long ev[2];
	HIPCHK(c, hipMemcpy(ev, c->evals.get<unsigned long long>() + 8, sizeof ev, hipMemcpyDeviceToHost));
	out->evals_prior = ev[0]; out->pixels_prior = ev[1];
	return HCMVS_OK;
}

// ---- geometric consistency ----

void hcmvs_default_geo_params(hcmvs_geo_params* p) {
	if (!p) return;
	p->on = 0; p->para_tapa = 0.25f; p->para_tapa2 = 0.15f; p->txthreshold = 150.f; p->txthreshold2 = 160.f; // DensifyPointCloud.cpp:176-181
	p->photo2geo = 2; p->max_px = 3.f;
}
int hcmvs_set_geo_params(hcmvs_ctx* c, const hcmvs_geo_params* p) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!p) return fail(c, HCMVS_ERR_INVALID, "set_geo_params: null argument");
	switch (est_check_geo_params(*p)) {
	case kGeoOk: break;
	case kGeoWeight: return fail(c, HCMVS_ERR_INVALID, "set_geo_params: para_tapa %g and para_tapa2 %g must lie in [0, 1]", (double)p->para_tapa, (double)p->para_tapa2);
	case kGeoThreshold: return fail(c, HCMVS_ERR_INVALID, "set_geo_params: txthreshold %g and txthreshold2 %g must be finite", (double)p->txthreshold, (double)p->txthreshold2);
	case kGeoMaxPx: return fail(c, HCMVS_ERR_INVALID, "set_geo_params: max_px %g is not a finite number > 0", (double)p->max_px);
	case kGeoPhoto2geo: return fail(c, HCMVS_ERR_INVALID, "set_geo_params: photo2geo %d is negative", p->photo2geo);
	}
	c->geo = *p;
	return HCMVS_OK;
}
int hcmvs_get_geo_stats(hcmvs_ctx* c, hcmvs_geo_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	memset(out, 0, sizeof *out);
	if (!c->haveStats) return fail(c, HCMVS_ERR_INVALID, "get_geo_stats: no estimate has run");
	if (!c->haveGeoStats) return HCMVS_OK; // the term was active for no item of the last estimate: all zero
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	unsigned long long ev[2];
	HIPCHK(c, hipMemcpy(ev, c->evals.get<unsigned long long>() + 10, sizeof ev, hipMemcpyDeviceToHost));
	out->evals_geo = ev[0]; out->pixels_geo = ev[1];
	return HCMVS_OK;
}

// ---- view spread (DensifyPointCloud --n-viewspread, DepthMap.cpp:1504-1608) ----

// ---- plane priors (DepthMapsData::GenerateDepthPrior, SceneDensify.cpp:1550-1950) ----

void hcmvs_default_plane_prior_params(hcmvs_plane_prior_params* p) {
	if (!p) return;
	memset(p, 0, sizeof *p);
	p->region_label = 255; p->conf_max = 0.18f; p->planarity_min = 0.3f; p->n_neighbors = 10; // SceneDensify.cpp:1625, :1648-1681
	p->probability = 0.01f; p->min_points_div = 80.f; p->epsilon_mul = 2.f;                    // DensifyPointCloud.cpp --ransac-*
	p->normal_threshold = 0.25f; p->max_rounds = 256; p->seed = 1;
	p->cluster_mul = 0.f; // clustering off: what the call computed before it had the field
	p->refit_iters = 0;   // no refit: likewise
}
int hcmvs_set_prior_region(hcmvs_ctx* c, uint32_t id, const uint16_t* labels, int32_t lw, int32_t lh, int32_t region_label) {
	if (!c) return HCMVS_ERR_INVALID;
	View* pv = find_view(c, "set_prior_region", id);
	if (!pv) return HCMVS_ERR_INVALID;
	View& v = *pv;
	HIPCHK(c, hipSetDevice(c->device));
	if (!labels) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		v.region.reset();
		return HCMVS_OK;
	}
	if (v.rescaled) return fail(c, HCMVS_ERR_INVALID, "set_prior_region: view %u was made by hcmvs_rescale_view: only a reference view has a prior", id);
	if (lw < 1 || lh < 1 || lw > 65536 || lh > 65536) return fail(c, HCMVS_ERR_INVALID, "set_prior_region: bad label image %dx%d (view %u)", lw, lh, id);
	// the ignore mask's resize: the region is where that mask would be 0 (a label outside 0 .. 65535 matches no 16-bit value)
	const bool matches = region_label >= 0 && region_label <= 65535;
	const size_t imgBytes = (size_t)lw * lh * sizeof(uint16_t);
	Carve cv;
	const size_t oImg = cv(imgBytes), oLab = cv(2 * sizeof(int32_t));
	HIPCHK(c, c->maskStage.reserve(cv.size, c->stream));
	HIPCHK(c, v.region.reserve((size_t)v.w * v.h, c->stream));
	const int rc = upload_staged(c, c->maskStage.get() + oImg, labels, imgBytes);
	if (rc) return rc;
	int32_t* dLabel = (int32_t*)(c->maskStage.get() + oLab);
	if (matches) HIPCHK(c, hipMemcpyAsync(dLabel, &region_label, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
	launch_ignore_mask((const uint16_t*)(c->maskStage.get() + oImg), lw, lh, dLabel, matches ? 1 : 0, v.region.get<uint8_t>(), v.w, v.h, c->stream);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (region_label and the staging go on being used by the next call)
	return HCMVS_OK;
}
int hcmvs_get_prior_region(hcmvs_ctx* c, uint32_t id, uint8_t* region) {
	if (!c || !region) return HCMVS_ERR_INVALID;
	const View* pv = find_view(c, "get_prior_region", id);
	if (!pv) return HCMVS_ERR_INVALID;
	const size_t n = (size_t)pv->w * pv->h;
	if (!pv->region.capacity()) { memset(region, 0, n); return HCMVS_OK; }
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(region, pv->region.get(), n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	for (size_t i = 0; i < n; ++i) region[i] = region[i] ? 0 : 1;
	return HCMVS_OK;
}
int hcmvs_generate_plane_prior_device(hcmvs_ctx* c, uint32_t id, const float* d_depth, const float* d_normal, const float* d_conf,
                                      const hcmvs_plane_prior_params* params, float* d_prior, float* d_prior_normal, hcmvs_prior_plane* planes,
                                      hcmvs_plane_prior_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	const View* pv = find_view(c, "generate_plane_prior", id);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	const PriorGenArgs args = {(uintptr_t)d_depth, (uintptr_t)d_normal, (uintptr_t)d_conf, (uintptr_t)d_prior, (uintptr_t)d_prior_normal, v.w, v.h, v.K, params};
	const std::string why = prior_gen_check(args);
	if (!why.empty()) return fail(c, HCMVS_ERR_INVALID, "generate_plane_prior: %s (view %u)", why.c_str(), id);
	HIPCHK(c, hipSetDevice(c->device));
	hcmvs_plane_prior_stats st;
	std::string err;
	const int rc = generate_plane_prior_device(v.w, v.h, v.K, v.region.capacity() ? v.region.get<uint8_t>() : nullptr, d_depth, d_normal, d_conf, *params, d_prior,
	                                           d_prior_normal, planes, st, c->priorGenKept, c->priorTrace, c->stream, err);
	if (rc) { c->priorTrace = PriorGenTrace(); return fail(c, HCMVS_ERR_HIP, "%s", err.c_str()); }
	if (stats) *stats = st;
	return HCMVS_OK;
}
int hcmvs_get_plane_prior_trace(hcmvs_ctx* c, uint8_t* stage, int32_t* assignment, int32_t* rounds, int32_t rounds_capacity, int32_t* n_rounds) {
	if (!c) return HCMVS_ERR_INVALID;
	const PriorGenTrace& t = c->priorTrace;
	if (rounds && rounds_capacity < 0) return fail(c, HCMVS_ERR_INVALID, "get_plane_prior_trace: negative capacity");
	const size_t px = (size_t)t.w * t.h, nRounds = t.rounds.size() / 6;
	if (n_rounds) *n_rounds = (int32_t)nRounds;
	if (rounds) memcpy(rounds, t.rounds.data(), sizeof(int32_t) * 6 * std::min(nRounds, (size_t)rounds_capacity));
	if (!stage && !assignment) return HCMVS_OK;
	if (!t.valid) return fail(c, HCMVS_ERR_INVALID, "get_plane_prior_trace: no hcmvs_generate_plane_prior_device has looked at a region");
	HIPCHK(c, hipSetDevice(c->device));
	const char* b = c->priorGenKept.get();
	if (stage) HIPCHK(c, hipMemcpyAsync(stage, b + t.lay.stage, px, hipMemcpyDeviceToHost, c->stream));
	std::vector<int32_t> pix, asg;
	if (assignment && t.n0) {
		pix.resize(t.n0); asg.resize(t.n0);
		HIPCHK(c, hipMemcpyAsync(pix.data(), b + t.lay.pixA, t.n0 * 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipMemcpyAsync(asg.data(), b + t.lay.assigned, t.n0 * 4, hipMemcpyDeviceToHost, c->stream));
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (assignment) {
		for (size_t i = 0; i < px; ++i) assignment[i] = -1;
		for (size_t i = 0; i < t.n0; ++i) assignment[pix[i]] = asg[i];
	}
	return HCMVS_OK;
}
int hcmvs_get_plane_prior_cluster_trace(hcmvs_ctx* c, int32_t* clusters, int32_t capacity, int32_t* n_rounds) {
	if (!c) return HCMVS_ERR_INVALID;
	const PriorGenTrace& t = c->priorTrace;
	if (clusters && capacity < 0) return fail(c, HCMVS_ERR_INVALID, "get_plane_prior_cluster_trace: negative capacity");
	const size_t nRounds = t.clusters.size() / 4;
	if (n_rounds) *n_rounds = (int32_t)nRounds;
	if (clusters) memcpy(clusters, t.clusters.data(), sizeof(int32_t) * 4 * std::min(nRounds, (size_t)capacity));
	return HCMVS_OK;
}
int hcmvs_get_plane_prior_refit_trace(hcmvs_ctx* c, int32_t* steps, float* planes, int32_t capacity, int32_t* n_rounds) {
	if (!c) return HCMVS_ERR_INVALID;
	const PriorGenTrace& t = c->priorTrace;
	if ((steps || planes) && capacity < 0) return fail(c, HCMVS_ERR_INVALID, "get_plane_prior_refit_trace: negative capacity");
	const size_t nRounds = t.refits.size() / 6;
	if (n_rounds) *n_rounds = (int32_t)nRounds;
	if (steps) memcpy(steps, t.refits.data(), sizeof(int32_t) * 6 * std::min(nRounds, (size_t)capacity));
	if (planes) memcpy(planes, t.refitPlanes.data(), sizeof(float) * 4 * std::min(nRounds, (size_t)capacity));
	return HCMVS_OK;
}
int hcmvs_get_plane_prior_refit_stats(hcmvs_ctx* c, hcmvs_plane_prior_refit_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	*out = c->priorTrace.refitStats;
	return HCMVS_OK;
}

int hcmvs_set_viewspread(hcmvs_ctx* c, int32_t on) {
	if (!c) return HCMVS_ERR_INVALID;
	c->viewspread = on != 0;
	return HCMVS_OK;
}
int hcmvs_set_spread_maps_device(hcmvs_ctx* c, uint32_t id, const float* d_depth, const float* d_normal, const float* d_conf) {
	if (!c) return HCMVS_ERR_INVALID;
	View* pv = find_view(c, "set_spread_maps", id);
	if (!pv) return HCMVS_ERR_INVALID;
	View& v = *pv;
	if (!d_depth && !d_normal && !d_conf) { v.sDepth = v.sNormal = v.sConf = nullptr; return HCMVS_OK; }
	if (!d_depth || !d_normal || !d_conf) return fail(c, HCMVS_ERR_INVALID, "set_spread_maps: view %u: depth, normal and conf are all needed (or all NULL)", id);
	if (v.rescaled) return fail(c, HCMVS_ERR_INVALID, "set_spread_maps: view %u was made by hcmvs_rescale_view: a resampled view has no maps of its size and never spreads", id);
	v.sDepth = d_depth; v.sNormal = d_normal; v.sConf = d_conf;
	return HCMVS_OK;
}
int hcmvs_get_spread_stats(hcmvs_ctx* c, hcmvs_spread_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	memset(out, 0, sizeof *out);
	if (!c->haveStats) return fail(c, HCMVS_ERR_INVALID, "get_spread_stats: no estimate has run");
	if (!c->haveSpreadStats) return HCMVS_OK; // the last estimate had no view spread to do: all zero
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	unsigned long long ev[8];
	HIPCHK(c, hipMemcpy(ev, c->evals.get(), 64, hipMemcpyDeviceToHost));
	out->slots_scored = ev[4]; out->slots_accepted = ev[5]; out->slots_dropped = ev[6]; out->candidates_outside = ev[7];
	return HCMVS_OK;
}

int hcmvs_estimate(hcmvs_ctx* c, uint32_t ref_id, const uint32_t* src_ids, int32_t n_src, const hcmvs_params* p, float d_min,
                   float d_max, float* depth, float* normal, float* conf) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!depth || !normal || !conf) return fail(c, HCMVS_ERR_INVALID, "estimate: null map buffer");
	const View* ref = find_view(c, "estimate", ref_id);
	if (!ref) return HCMVS_ERR_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)ref->w * ref->h;
	hipStream_t s = c->stream;
	HIPCHK(c, c->sDepth.reserve(n * 4, s));
	HIPCHK(c, c->sNormal.reserve(n * 12, s));
	HIPCHK(c, c->sConf.reserve(n * 4, s));
	float *sDepth = c->sDepth.get<float>(), *sNormal = c->sNormal.get<float>(), *sConf = c->sConf.get<float>();
	HIPCHK(c, hipMemcpyAsync(sDepth, depth, n * 4, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemcpyAsync(sNormal, normal, n * 12, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemcpyAsync(sConf, conf, n * 4, hipMemcpyHostToDevice, s));
	int rc = hcmvs_estimate_device(c, ref_id, src_ids, n_src, p, d_min, d_max, sDepth, sNormal, sConf);
	if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(depth, sDepth, n * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipMemcpyAsync(normal, sNormal, n * 12, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipMemcpyAsync(conf, sConf, n * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s));
	hcmvs_stats st;
	return hcmvs_get_stats(c, &st); // surfaces a sweep timeout as an error
}

int hcmvs_splat_points(int32_t W, int32_t H, const double K[9], const double R[9], const double C[3], const float* pts, int32_t n, float* depth,
                       float* normal, float* d_min, float* d_max) {
	if (!K || !R || !C || !pts || !depth || !normal || !d_min || !d_max || n < 1 || W < 1 || H < 1) return HCMVS_ERR_INVALID;
	std::vector<InitSplat> table; // the per-point set-up (init_plan.h); the device form rasterises the same table
	float dmin, dmax;
	splat_plan(K, R, C, pts, n, table, &dmin, &dmax);
	memset(depth, 0, sizeof(float) * (size_t)W * H);
	for (const InitSplat& p : table) { // SceneDensify.cpp:789-806
		const InitBox bx = splat_box(p, W, H);
		for (int yy = bx.y0; yy < bx.y1; ++yy)
			for (int xx = bx.x0; xx < bx.x1; ++xx) {
				depth[(size_t)yy * W + xx] = p.d;
				float* nn = normal + 3 * ((size_t)yy * W + xx);
				nn[0] = nn[1] = nn[2] = 0.f;
			}
	}
	*d_min = dmin * 0.9f;
	*d_max = dmax * 1.1f;
	return HCMVS_OK;
}
int hcmvs_splat_init(hcmvs_ctx* c, uint32_t id, const float* pts, int32_t n, float* depth, float* normal, float* d_min,
                     float* d_max) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!pts || !depth || !normal || !d_min || !d_max || n < 1) return fail(c, HCMVS_ERR_INVALID, "splat_init: bad arguments");
	const View* pv = find_view(c, "splat_init", id);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	return hcmvs_splat_points(v.w, v.h, v.K, v.R, v.C, pts, n, depth, normal, d_min, d_max);
}

int hcmvs_triangulate_points(int32_t W, int32_t H, const double K[9], const double R[9], const double C[3], const float* pts,
                             int32_t n, float avg_depth, int32_t add_corners, float* depth, float* normal, float* d_min, float* d_max) {
	if (!K || !R || !C || !pts || !depth || !normal || !d_min || !d_max || n < 1 || W < 1 || H < 1) return HCMVS_ERR_INVALID;
	float lo = 0.f, hi = 0.f;
	if (!hcmvs::triangulate_init(W, H, K, R, C, pts, n, avg_depth, add_corners != 0, depth, normal, &lo, &hi)) return HCMVS_ERR_INVALID;
	*d_min = lo * 0.9f; // SceneDensify.cpp:524-525
	*d_max = hi * 1.1f;
	return HCMVS_OK;
}
int hcmvs_triangulate_init(hcmvs_ctx* c, uint32_t id, const float* pts, int32_t n, float avg_depth, int32_t add_corners, float* depth,
                           float* normal, float* d_min, float* d_max) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!pts || !depth || !normal || !d_min || !d_max || n < 1) return fail(c, HCMVS_ERR_INVALID, "triangulate_init: bad arguments");
	const View* pv = find_view(c, "triangulate_init", id);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	if (hcmvs_triangulate_points(v.w, v.h, v.K, v.R, v.C, pts, n, avg_depth, add_corners, depth, normal, d_min, d_max) != HCMVS_OK)
		return fail(c, HCMVS_ERR_INVALID, "triangulate_init: no sparse point in front of view %u", id);
	return HCMVS_OK;
}

// what the two device initialisations refuse before any work: the view, or null with the failure recorded
static const View* init_device_args(hcmvs_ctx* c, const char* who, uint32_t id, const float* pts, int32_t n, const float* d_depth, const float* d_normal,
                                    const float* d_min, const float* d_max) {
	if (!pts || !d_depth || !d_normal || !d_min || !d_max || n < 1) { fail(c, HCMVS_ERR_INVALID, "%s: bad arguments (null pointer or n_points < 1)", who); return nullptr; }
	const View* v = find_view(c, who, id);
	if (!v) return nullptr;
	for (size_t i = 0; i < (size_t)n * 3; ++i)
		if (!std::isfinite(pts[i])) { fail(c, HCMVS_ERR_INVALID, "%s: coordinate %d of point %zu is not finite", who, (int)(i % 3), i / 3); return nullptr; }
	return v;
}

// The device half of the two initialisations: the table (tableBytes at `table`) and the tile lists go through the context's page-locked
// staging into its grow-only buffer, then one kernel writes every pixel of the caller's maps.  Enqueued on the context's stream, not
// synchronised; the staging is rewritten only after the event that marks its copy.
static int init_enqueue(hcmvs_ctx* c, const char* who, bool triangles, const View& v, const void* table, size_t tableBytes, const InitTiling& t,
                        float fx, float fy, float cx, float cy, float* d_depth, float* d_normal) {
	HIPCHK(c, hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const size_t nTiles = (size_t)t.tilesX * t.tilesY;
	const InitLayout l = init_layout(tableBytes, nTiles, t.items.size());
	HIPCHK(c, c->initCopied.ensure());
	for (Event& e : c->initEv) HIPCHK(c, e.ensure());
	if (c->initInFlight) { HIPCHK(c, hipEventSynchronize(c->initCopied.get())); c->initInFlight = false; } // the previous call's tables have left the staging
	if (c->initPinned.capacity() < l.bytes) {
		const size_t cap = std::max(l.bytes + l.bytes / 2, (size_t)1 << 20);
		if (c->initPinned.reserve(cap) != hipSuccess) return fail(c, HCMVS_ERR_HIP, "%s: no page-locked staging of %zu bytes", who, cap);
	}
	HIPCHK(c, c->initBuf.reserve(l.bytes, s));
	char* h = c->initPinned.get();
	memset(h + l.counters, 0, 2 * sizeof(uint64_t));
	if (tableBytes) memcpy(h + l.table, table, tableBytes);
	memcpy(h + l.first, t.first.data(), (nTiles + 1) * sizeof(uint32_t));
	if (!t.items.empty()) memcpy(h + l.items, t.items.data(), t.items.size() * sizeof(uint32_t));
	char* d = c->initBuf.get();
	HIPCHK(c, hipMemcpyAsync(d, h, l.bytes, hipMemcpyHostToDevice, s)); // same stream: the previous call's kernel is done with the buffer
	HIPCHK(c, hipEventRecord(c->initCopied.get(), s));
	c->initInFlight = true;
	InitRaster r;
	r.W = v.w; r.H = v.h; r.tilesX = t.tilesX; r.tilesY = t.tilesY;
	r.fx = fx; r.fy = fy; r.cx = cx; r.cy = cy;
	r.first = (const uint32_t*)(d + l.first); r.items = (const uint32_t*)(d + l.items);
	r.depth = d_depth; r.normal = d_normal;
	r.counters = (unsigned long long*)(d + l.counters);
	HIPCHK(c, hipEventRecord(c->initEv[0].get(), s));
	if (triangles) launch_init_triangles(r, (const InitFace*)(d + l.table), s);
	else launch_init_splats(r, (const InitSplatBox*)(d + l.table), s);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(c->initEv[1].get(), s));
	c->initStats.n_tile_entries = t.items.size();
	c->initStats.device_bytes = l.bytes;
	c->haveInitStats = true;
	return HCMVS_OK;
}

static float ms_since(std::chrono::steady_clock::time_point t0) {
	return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int hcmvs_triangulate_init_device(hcmvs_ctx* c, uint32_t id, const float* pts, int32_t n, float avg_depth, int32_t add_corners, float* d_depth,
                                  float* d_normal, float* d_min, float* d_max) {
	if (!c) return HCMVS_ERR_INVALID;
	const View* pv = init_device_args(c, "triangulate_init_device", id, pts, n, d_depth, d_normal, d_min, d_max);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	const auto t0 = std::chrono::steady_clock::now();
	InitTriTable tab;
	if (!hcmvs::triangulate_plan(v.w, v.h, v.K, v.R, v.C, pts, n, avg_depth, add_corners != 0, tab))
		return fail(c, HCMVS_ERR_INVALID, "triangulate_init_device: no sparse point in front of view %u", id);
	InitTiling tiles;
	if (!bin_tiles(v.w, v.h, tab.faces.size(), [&](size_t i) { return face_box(tab.faces[i]); }, tiles))
		return fail(c, HCMVS_ERR_INVALID, "triangulate_init_device: the tile lists of view %u pass 2^31 entries", id);
	c->haveInitStats = false;
	c->initStats = hcmvs_init_stats();
	c->initStats.n_used = (uint64_t)tab.nUsed; c->initStats.n_faces = tab.faces.size();
	c->initStats.ms_host = ms_since(t0);
	const int rc = init_enqueue(c, "triangulate_init_device", true, v, tab.faces.data(), tab.faces.size() * sizeof(InitFace), tiles, tab.fx, tab.fy, tab.cx,
	                            tab.cy, d_depth, d_normal);
	if (rc) return rc;
	*d_min = tab.lo * 0.9f; // SceneDensify.cpp:524-525
	*d_max = tab.hi * 1.1f;
	return HCMVS_OK;
}

int hcmvs_splat_init_device(hcmvs_ctx* c, uint32_t id, const float* pts, int32_t n, float* d_depth, float* d_normal, float* d_min, float* d_max) {
	if (!c) return HCMVS_ERR_INVALID;
	const View* pv = init_device_args(c, "splat_init_device", id, pts, n, d_depth, d_normal, d_min, d_max);
	if (!pv) return HCMVS_ERR_INVALID;
	const View& v = *pv;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<InitSplat> tab;
	float dmin, dmax;
	splat_plan(v.K, v.R, v.C, pts, n, tab, &dmin, &dmax);
	std::vector<InitSplatBox> boxes(tab.size());
	for (size_t i = 0; i < tab.size(); ++i) {
		const InitBox b = splat_box(tab[i], v.w, v.h);
		boxes[i] = {b.x0, b.y0, b.x1, b.y1, tab[i].d};
	}
	InitTiling tiles;
	if (!bin_tiles(v.w, v.h, boxes.size(), [&](size_t i) { return InitBox{boxes[i].x0, boxes[i].y0, boxes[i].x1, boxes[i].y1}; }, tiles))
		return fail(c, HCMVS_ERR_INVALID, "splat_init_device: the tile lists of view %u pass 2^31 entries", id);
	c->haveInitStats = false;
	c->initStats = hcmvs_init_stats();
	c->initStats.n_used = tab.size();
	c->initStats.ms_host = ms_since(t0);
	const int rc = init_enqueue(c, "splat_init_device", false, v, boxes.data(), boxes.size() * sizeof(InitSplatBox), tiles, 0.f, 0.f, 0.f, 0.f, d_depth, d_normal);
	if (rc) return rc;
	*d_min = dmin * 0.9f;
	*d_max = dmax * 1.1f;
	return HCMVS_OK;
}

int hcmvs_get_init_stats(hcmvs_ctx* c, hcmvs_init_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	if (!c->haveInitStats) return fail(c, HCMVS_ERR_INVALID, "get_init_stats: no device initialisation has run on this context");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	unsigned long long counters[2] = {0, 0};
	HIPCHK(c, hipMemcpy(counters, c->initBuf.get(), sizeof counters, hipMemcpyDeviceToHost)); // InitLayout: the counters open the buffer
	HIPCHK(c, hipEventElapsedTime(&c->initStats.ms_device, c->initEv[0].get(), c->initEv[1].get()));
	c->initStats.covered_pixels = counters[0]; c->initStats.cover_hits = counters[1];
	*out = c->initStats;
	return HCMVS_OK;
}

// cv::resize INTER_AREA, enlarging (OpenCV 4.2 imgproc/src/resize.cpp: the bilinear kernel driven by "area mode" tables):
// per destination column / row the left / upper source index and the weight of its right / lower partner
int hcmvs_resize_area_up(const float* src, int32_t sw, int32_t sh, int32_t ch, float* dst, int32_t dw, int32_t dh) {
	if (!src || !dst || sw < 1 || sh < 1 || ch < 1 || dw < sw || dh < sh) return HCMVS_ERR_INVALID;
	struct Tab { std::vector<int> ofs; std::vector<float> w; };
	auto table = [](int ssize, int dsize, bool columns) {
		Tab t; t.ofs.resize((size_t)dsize); t.w.resize((size_t)dsize);
		const double scale = (double)ssize / dsize, inv = (double)dsize / ssize;
		for (int d = 0; d < dsize; ++d) {
			int s = (int)std::floor(d * scale);
			float f = (float)((d + 1) - (s + 1) * inv);
			f = f <= 0 ? 0.f : f - std::floor(f);
			if (columns && s >= ssize - 1) { f = 0.f; s = ssize - 1; } // no right partner: the sample alone (HResizeLinear past xmax)
			t.ofs[(size_t)d] = s; t.w[(size_t)d] = f;
		}
		return t;
	};
	const Tab tx = table(sw, dw, true), ty = table(sh, dh, false);
	std::vector<float> row0((size_t)dw * ch), row1((size_t)dw * ch);
	auto hresize = [&](int sy, std::vector<float>& out) {
		const float* S = src + (size_t)sy * sw * ch;
		for (int x = 0; x < dw; ++x) {
			const int sx = tx.ofs[(size_t)x];
			const float a1 = tx.w[(size_t)x], a0 = 1.f - a1;
			for (int c = 0; c < ch; ++c)
				out[(size_t)x * ch + c] = sx + 1 >= sw ? S[(size_t)sx * ch + c] : S[(size_t)sx * ch + c] * a0 + S[(size_t)(sx + 1) * ch + c] * a1;
		}
	};
	int have0 = -1, have1 = -1;
	for (int y = 0; y < dh; ++y) {
		const int r0 = std::min(std::max(ty.ofs[(size_t)y], 0), sh - 1), r1 = std::min(std::max(ty.ofs[(size_t)y] + 1, 0), sh - 1);
		if (have0 != r0) { if (have1 == r0) { row0.swap(row1); std::swap(have0, have1); } else { hresize(r0, row0); have0 = r0; } }
		if (have1 != r1) { hresize(r1, row1); have1 = r1; }
		const float b1 = ty.w[(size_t)y], b0 = 1.f - b1;
		float* D = dst + (size_t)y * dw * ch;
		for (size_t k = 0; k < (size_t)dw * ch; ++k) D[k] = row0[k] * b0 + row1[k] * b1;
	}
	return HCMVS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the hand-off between pyramid levels (handoff_device.h states the rule, handoff_plan.h the checks and the launch plan)

static std::vector<HandoffArgs> handoff_args(const hcmvs_handoff_item* items, int32_t n) {
	std::vector<HandoffArgs> a;
	if (!items || n < 1 || n > kHandoffMaxItems) return a; // handoff_check reports it
	a.resize((size_t)n);
	for (int i = 0; i < n; ++i)
		a[(size_t)i] = {(uintptr_t)items[i].src_depth, (uintptr_t)items[i].src_normal, (uintptr_t)items[i].dst_depth, (uintptr_t)items[i].dst_normal,
		                items[i].src_w, items[i].src_h, items[i].dst_w, items[i].dst_h, items[i].d_min, items[i].d_max};
	return a;
}
static void handoff_report(hcmvs_handoff_item& it, int mode, const HandoffResult& r) {
	it.status = handoff_finish(mode, r, &it.d_min, &it.d_max) ? HCMVS_HANDOFF_OK : HCMVS_HANDOFF_EMPTY;
	it.n_valid = r.valid; it.n_clamped = r.clamped; it.n_rescaled = r.rescaled;
}

int hcmvs_handoff_maps(hcmvs_handoff_item* items, int32_t n, int32_t mode) {
	const std::vector<HandoffArgs> args = handoff_args(items, n);
	if (!handoff_check(args.empty() ? nullptr : args.data(), n, mode).empty()) return HCMVS_ERR_INVALID;
	for (int i = 0; i < n; ++i) {
		hcmvs_handoff_item& it = items[i];
		HandoffResult r;
		it.status = handoff_host(mode, handoff_geom(it.src_w, it.src_h, it.dst_w, it.dst_h), it.src_depth, it.src_normal, it.dst_depth, it.dst_normal, &it.d_min,
		                         &it.d_max, r) ? HCMVS_HANDOFF_OK : HCMVS_HANDOFF_EMPTY;
		it.n_valid = r.valid; it.n_clamped = r.clamped; it.n_rescaled = r.rescaled;
	}
	return HCMVS_OK;
}

int hcmvs_handoff_maps_device(hcmvs_ctx* c, hcmvs_handoff_item* items, int32_t n, int32_t mode) {
	if (!c) return HCMVS_ERR_INVALID;
	const std::vector<HandoffArgs> args = handoff_args(items, n);
	const std::string why = handoff_check(args.empty() ? nullptr : args.data(), n, mode);
	if (!why.empty()) return fail(c, HCMVS_ERR_INVALID, "handoff_maps_device: %s", why.c_str());
	HIPCHK(c, hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const std::vector<int32_t> first = handoff_first(args.data(), n);
	const HandoffLayout l = handoff_layout(n, (size_t)first[(size_t)n]);
	for (Event& e : c->handoffEv) HIPCHK(c, e.ensure());
	if (c->handoffPinned.reserve(handoff_layout(kHandoffMaxItems, 0).staged) != hipSuccess) return fail(c, HCMVS_ERR_HIP, "handoff_maps_device: no page-locked staging");
	HIPCHK(c, c->handoffBuf.reserve(l.bytes, s));
	char* h = c->handoffPinned.get();
	HandoffResult* hr = (HandoffResult*)(h + l.results);
	HandoffItem* hi = (HandoffItem*)(h + l.items);
	uint64_t pixels = 0;
	for (int i = 0; i < n; ++i) {
		hr[i] = HandoffResult(); // written by the device
		hi[i] = {items[i].src_depth, items[i].src_normal, items[i].dst_depth, items[i].dst_normal, handoff_geom(items[i].src_w, items[i].src_h, items[i].dst_w, items[i].dst_h)};
		pixels += (uint64_t)items[i].dst_w * items[i].dst_h;
	}
	memcpy(h + l.first, first.data(), first.size() * sizeof(int32_t));
	char* d = c->handoffBuf.get();
	HIPCHK(c, hipMemcpyAsync(d, h, l.staged, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipEventRecord(c->handoffEv[0].get(), s));
	launch_handoff(mode, (const HandoffItem*)(d + l.items), (const int32_t*)(d + l.first), n, first[(size_t)n], (HandoffResult*)(d + l.partials),
	               (HandoffResult*)(d + l.results), s);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(c->handoffEv[1].get(), s));
	HIPCHK(c, hipMemcpyAsync(hr, d + l.results, (size_t)n * sizeof(HandoffResult), hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s)); // the one synchronisation of the call: the ranges are final on return
	hcmvs_handoff_stats st = hcmvs_handoff_stats();
	st.n_pixels = pixels; st.n_items = n;
	for (int i = 0; i < n; ++i) {
		handoff_report(items[i], mode, hr[i]);
		st.n_valid += items[i].n_valid; st.n_clamped += items[i].n_clamped; st.n_rescaled += items[i].n_rescaled;
		st.n_empty += items[i].status == HCMVS_HANDOFF_EMPTY;
	}
	c->handoffStats = st;
	c->haveHandoffStats = true;
	return HCMVS_OK;
}

int hcmvs_get_handoff_stats(hcmvs_ctx* c, hcmvs_handoff_stats* out) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	if (!c->haveHandoffStats) return fail(c, HCMVS_ERR_INVALID, "get_handoff_stats: no device hand-off has run on this context");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipEventElapsedTime(&c->handoffStats.ms_device, c->handoffEv[0].get(), c->handoffEv[1].get())); // the call synchronised: both events have passed
	*out = c->handoffStats;
	return HCMVS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the speckle filter (speckle_plan.h states the rule, the checks and the plan; speckle_host.h the CPU form)

static std::vector<SpeckleArgs> speckle_args(const hcmvs_speckle_item* items, int32_t n) {
	std::vector<SpeckleArgs> a;
	if (!items || n < 1 || n > kSpeckleMaxItems) return a; // speckle_check reports it
	a.resize((size_t)n);
	for (int i = 0; i < n; ++i)
		a[(size_t)i] = {(uintptr_t)items[i].d_depth, (uintptr_t)items[i].d_normal, (uintptr_t)items[i].d_conf, (uintptr_t)items[i].d_labels, items[i].width, items[i].height};
	return a;
}
static void speckle_report(const SpeckleResult& r, hcmvs_speckle_stats* st) {
	st->n_valid = r.valid; st->n_removed = r.removed; st->n_segments = r.segments; st->n_small = r.small; st->largest = r.largest;
}

int hcmvs_remove_speckles(int32_t w, int32_t h, float* depth, float* normal, float* conf, int32_t* labels, float thr, uint32_t speckle_size, hcmvs_speckle_stats* stats) {
	const SpeckleArgs a = {(uintptr_t)depth, (uintptr_t)normal, (uintptr_t)conf, (uintptr_t)labels, w, h};
	if (!speckle_check(&a, 1, thr).empty()) return HCMVS_ERR_INVALID;
	SpeckleResult r = SpeckleResult();
	speckle_host(w, h, depth, normal, conf, labels, thr, speckle_size, r);
	if (stats) { *stats = hcmvs_speckle_stats(); speckle_report(r, stats); }
	return HCMVS_OK;
}

int hcmvs_remove_speckles_batch_device(hcmvs_ctx* c, const hcmvs_speckle_item* items, int32_t n, float thr, uint32_t speckle_size, hcmvs_speckle_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	const std::vector<SpeckleArgs> args = speckle_args(items, n);
	const SpeckleArgs none = SpeckleArgs(); // items given, n_items out of range: the check reports the count and reads nothing
	const std::string why = speckle_check(!args.empty() ? args.data() : items ? &none : nullptr, n, thr);
	if (!why.empty()) return fail(c, HCMVS_ERR_INVALID, "remove_speckles_batch_device: %s", why.c_str());
	const SpeckleTiles tiles = speckle_tiles(args.data(), n);
	if (!speckle_grid_fits(tiles)) return fail(c, HCMVS_ERR_INVALID, "remove_speckles_batch_device: the batch has 2^31 tiles or more");
	HIPCHK(c, hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const int nTiles = (int)tiles.first[(size_t)n];
	const SpeckleLayout l = speckle_layout(n, (size_t)nTiles, (size_t)tiles.pixel0[(size_t)n]);
	for (Event& e : c->speckleEv) HIPCHK(c, e.ensure());
	if (c->specklePinned.reserve(speckle_layout(kSpeckleMaxItems, 0, 0).staged) != hipSuccess) return fail(c, HCMVS_ERR_HIP, "remove_speckles_batch_device: no page-locked staging");
	HIPCHK(c, c->speckleBuf.reserve(l.bytes, s));
	char* h = c->specklePinned.get();
	char* d = c->speckleBuf.get();
	SpeckleResult* hr = (SpeckleResult*)(h + l.result);
	SpeckleItem* hi = (SpeckleItem*)(h + l.items);
	int32_t* hf = (int32_t*)(h + l.first);
	*hr = SpeckleResult(); // the error word starts clear
	for (int i = 0; i < n; ++i) {
		hi[i] = {items[i].d_depth, items[i].d_normal, items[i].d_conf, items[i].d_labels, (int32_t*)(d + l.labels) + tiles.pixel0[(size_t)i],
		         (int32_t*)(d + l.sizes) + tiles.pixel0[(size_t)i], items[i].width, items[i].height, speckle_tiles_x(items[i].width), 0};
		hf[i] = (int32_t)tiles.first[(size_t)i];
	}
	hf[n] = nTiles;
	HIPCHK(c, hipMemcpyAsync(d, h, l.staged, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipEventRecord(c->speckleEv[0].get(), s));
	launch_speckle((const SpeckleItem*)(d + l.items), (const int32_t*)(d + l.first), n, nTiles, thr, speckle_size, (SpecklePartial*)(d + l.partials),
	               (SpeckleResult*)(d + l.result), s);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(c->speckleEv[1].get(), s));
	HIPCHK(c, hipMemcpyAsync(hr, d + l.result, sizeof(SpeckleResult), hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s)); // the one synchronisation of the call: the counters and the error word
	if (hr->error) return fail(c, HCMVS_ERR_INTERNAL, "remove_speckles_batch_device: a union-find loop ran past its bound; the maps of the call are not to be used");
	if (stats) {
		*stats = hcmvs_speckle_stats();
		speckle_report(*hr, stats);
		HIPCHK(c, hipEventElapsedTime(&stats->ms_device, c->speckleEv[0].get(), c->speckleEv[1].get()));
		stats->device_bytes = l.bytes;
	}
	return HCMVS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// filter / fuse

static int set_maps(hcmvs_ctx* c, uint32_t id, const float* depth, const float* normal, const float* conf, float dmin, float dmax, bool copy) {
	if (!c) return HCMVS_ERR_INVALID;
	View* pv = find_view(c, "set_depthmap", id);
	if (!pv) return HCMVS_ERR_INVALID;
	if (!depth || !conf) return fail(c, HCMVS_ERR_INVALID, "set_depthmap: null map");
	View& v = *pv;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	v.mDepth = v.mNormal = v.mConf = nullptr;
	v.depthMem.reset(); v.normalMem.reset(); v.confMem.reset(); // the old maps go before the new ones come
	const size_t n = (size_t)v.w * v.h;
	if (copy) {
		HIPCHK(c, v.depthMem.reserve(n * 4, c->stream));
		HIPCHK(c, v.confMem.reserve(n * 4, c->stream));
		v.mDepth = v.depthMem.get<float>(); v.mConf = v.confMem.get<float>();
		int rc = upload_staged(c, v.mDepth, depth, n * 4);
		if (!rc) rc = upload_staged(c, v.mConf, conf, n * 4);
		if (rc) return rc;
		if (normal) {
			HIPCHK(c, v.normalMem.reserve(n * 12, c->stream));
			v.mNormal = v.normalMem.get<float>();
			rc = upload_staged(c, v.mNormal, normal, n * 12);
			if (rc) return rc;
		}
	} else {
		v.mDepth = const_cast<float*>(depth); v.mNormal = const_cast<float*>(normal); v.mConf = const_cast<float*>(conf);
	}
	v.dMin = dmin; v.dMax = dmax;
	return HCMVS_OK;
}
int hcmvs_set_depthmap(hcmvs_ctx* c, uint32_t id, const float* depth, const float* normal, const float* conf, float d_min, float d_max) {
	return set_maps(c, id, depth, normal, conf, d_min, d_max, true);
}
int hcmvs_set_depthmap_device(hcmvs_ctx* c, uint32_t id, float* d_depth, const float* d_normal, const float* d_conf, float d_min, float d_max) {
	return set_maps(c, id, d_depth, d_normal, d_conf, d_min, d_max, false);
}
int hcmvs_get_depthmap(hcmvs_ctx* c, uint32_t id, float* depth, float* normal, float* conf) {
	if (!c) return HCMVS_ERR_INVALID;
	auto it = c->views.find(id);
	if (it == c->views.end() || !it->second.mDepth) return fail(c, HCMVS_ERR_INVALID, "get_depthmap: view %u has no maps", id);
	const View& v = it->second;
	const size_t n = (size_t)v.w * v.h;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (depth) HIPCHK(c, hipMemcpy(depth, v.mDepth, n * 4, hipMemcpyDeviceToHost));
	if (normal && v.mNormal) HIPCHK(c, hipMemcpy(normal, v.mNormal, n * 12, hipMemcpyDeviceToHost));
	if (conf) HIPCHK(c, hipMemcpy(conf, v.mConf, n * 4, hipMemcpyDeviceToHost));
	return HCMVS_OK;
}
int hcmvs_set_neighbors(hcmvs_ctx* c, uint32_t id, const uint32_t* ids, int32_t n) {
	if (!c) return HCMVS_ERR_INVALID;
	auto it = c->views.find(id);
	if (it == c->views.end() || n < 0 || n > 64 || (n > 0 && !ids)) return fail(c, HCMVS_ERR_INVALID, "set_neighbors: bad arguments for view %u", id);
	// any id a view could be registered under is taken (a neighbour need not be registered, nor have maps: the fuse, post-filter and filter
	// entries pass such an entry over); an id no view can have is refused here, so that the map table, which covers every id a list names,
	// stays within kMaxViewId entries
	for (int k = 0; k < n; ++k)
		if (ids[k] >= kMaxViewId) return fail(c, HCMVS_ERR_INVALID, "set_neighbors: neighbour id %u of view %u is not below %u", ids[k], id, kMaxViewId);
	View& v = it->second;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	v.dNeighbors.reset();
	v.neighbors.assign(ids, ids + n);
	if (n > 0) {
		HIPCHK(c, v.dNeighbors.reserve((size_t)n * 4, c->stream));
		HIPCHK(c, hipMemcpy(v.dNeighbors.get(), ids, (size_t)n * 4, hipMemcpyHostToDevice));
	}
	return HCMVS_OK;
}

static void fill_devmap(uint32_t id, const View& v, DevMap& m) {
	memset(&m, 0, sizeof m);
	m.id = id; m.w = v.w; m.h = v.h; m.nNeighbors = (int)v.neighbors.size();
	memcpy(m.K, v.K, sizeof m.K); memcpy(m.R, v.R, sizeof m.R); memcpy(m.C, v.C, sizeof m.C);
	double t[3];
	for (int i = 0; i < 3; ++i) t[i] = -(v.R[i * 3] * v.C[0] + v.R[i * 3 + 1] * v.C[1] + v.R[i * 3 + 2] * v.C[2]);
	for (int i = 0; i < 3; ++i) { // P = K [R | -R C], Camera.h:276-282
		for (int j = 0; j < 3; ++j) m.P[i * 4 + j] = v.K[i * 3] * v.R[j] + v.K[i * 3 + 1] * v.R[3 + j] + v.K[i * 3 + 2] * v.R[6 + j];
		m.P[i * 4 + 3] = v.K[i * 3] * t[0] + v.K[i * 3 + 1] * t[1] + v.K[i * 3 + 2] * t[2];
	}
	m.depth = v.mDepth; m.normal = v.mNormal; m.conf = v.mConf; m.bgr = v.bgr;
	m.neighbors = v.dNeighbors.get<uint32_t>(); m.dMin = v.dMin; m.dMax = v.dMax;
}
// device table indexed by image id (views without maps have depth == null).  It covers every id a registered neighbour list names as
// well: the fuse and post-filter kernels index it (and the chain's PfImage table, which has the same size) with A.neighbors[q] before
// they test depth, and the zeroed entry of an id that is not a registered view reads as "no maps".  hcmvs_set_neighbors bounds the ids.
// What the scene-level entries open with: the device, an idle stream, the table.
static int scene_prologue(hcmvs_ctx* c, std::vector<DevMap>& host) {
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	uint32_t maxId = 0;
	for (auto& kv : c->views) {
		if (kv.first > maxId) maxId = kv.first;
		for (uint32_t nb : kv.second.neighbors) if (nb > maxId) maxId = nb;
	}
	host.assign((size_t)maxId + 1, DevMap());
	for (auto& m : host) memset(&m, 0, sizeof m);
	for (auto& kv : c->views) fill_devmap(kv.first, kv.second, host[kv.first]);
	HIPCHK(c, c->dMaps.reserve(host.size() * sizeof(DevMap), c->stream));
	HIPCHK(c, hipMemcpy(c->dMaps.get(), host.data(), host.size() * sizeof(DevMap), hipMemcpyHostToDevice));
	HIPCHK(c, c->counters.reserve(8 * sizeof(unsigned long long), c->stream));
	return HCMVS_OK;
}

// the map table as the plans of fuse_plan.h see it
static std::vector<PlanMap> plan_maps(const hcmvs_ctx* c, const std::vector<DevMap>& host) {
	std::vector<PlanMap> maps(host.size());
	for (auto& kv : c->views) {
		PlanMap& m = maps[kv.first];
		m.pixels = (size_t)kv.second.w * kv.second.h; m.hasMaps = kv.second.mDepth != nullptr;
		m.nNeighbors = (int)kv.second.neighbors.size(); m.neighbors = kv.second.neighbors.data();
	}
	return maps;
}
// the dimensions of a fusion over `order` for the entry point `who`, or the failure when one of their limits is broken
static int fuse_call_dims(hcmvs_ctx* c, const char* who, const std::vector<PlanMap>& maps, const uint32_t* order, int n_order, FuseDims& d) {
	d = fuse_dims(maps, order, n_order);
	switch (d.broken) {
	case kFuseOk: return HCMVS_OK;
	case kFuseNoMaps: return fail(c, HCMVS_ERR_INVALID, "%s: view %u has no maps", who, order[d.at]);
	case kFuseTooManyNeighbors: return fail(c, HCMVS_ERR_INVALID, "%s: view %u has too many neighbours", who, order[d.at]);
	case kFuseStrideLimit: return fail(c, HCMVS_ERR_CAPACITY, "%s: maps of %zu pixels exceed the target tables (2^29 pixels)", who, d.stride);
	case kFuseTableLimit: break;
	}
	return fail(c, HCMVS_ERR_CAPACITY, "%s: %d neighbours of %zu pixels exceed the per-pass tables", who, d.maxNb, d.stride);
}

// the per-pass tables of a fusion from scratch (fuse_plan.h FuseCore) in device memory, and what every pass of the call has in common
struct FusePass {
	FusePass(char* b, const FuseCore& o, size_t stride)
	    : pending((uint32_t*)(b + o.pending)), settle(b + o.settle), ctl((uint32_t*)(b + o.ctl)), counters((unsigned long long*)(b + o.counters)),
	      status((uint32_t*)(b + o.status)), merged((uint32_t*)(b + o.merged)), flag((uint8_t*)(b + o.flag)), nv((uint32_t*)(b + o.nv)),
	      tb(fuse_tables((int32_t*)(b + o.targets), (uint32_t*)(b + o.head), (uint32_t*)(b + o.next), stride)) {}
	uint32_t* pending; void* settle; uint32_t* ctl; unsigned long long* counters; uint32_t* status; uint32_t* merged; uint8_t* flag; uint32_t* nv;
	FuseTables tb;
	float thDepth = 0.f, normalError = 0.f;
	int nMinViewsFuse = 0, vstride = 0;
};
// enqueues the pass of image A of a fusion from scratch.  oxyz .. oweights: where the pass leaves A's points (null: not wanted)
static int enqueue_fuse_pass(hcmvs_ctx* c, const DevMap& A, const FusePass& t, float* oxyz, float* onormal, uint8_t* obgr, uint32_t* oviews, float* oweights,
                             int order, bool wantPoints) {
	hipStream_t s = c->stream;
	HIPCHK(c, hipMemsetAsync(t.ctl, 0, kCtlBytes, s));
	HIPCHK(c, hipMemsetAsync(t.tb.head, 0xFF, (size_t)A.nNeighbors * t.tb.stride * 4, s)); // empty bidder lists
	launch_fuse_begin(A, c->dMaps.get<DevMap>(), t.tb, t.pending, t.ctl, t.flag, t.counters, t.thDepth, t.normalError, s);
	launch_fuse_pass(A, c->dMaps.get<DevMap>(), t.tb, t.pending, t.settle, t.ctl, oxyz, onormal, obgr, t.nv, t.flag, oviews, oweights, t.vstride, t.merged, t.nMinViewsFuse,
	                 order, t.counters, t.status, wantPoints, s);
	return HCMVS_OK;
}
// after the last pass of a fusion: the status words and nWords 64-bit words at dWords (counters or totals), once the stream is idle.
// HCMVS_ERR_TIMEOUT when a pass gave up.
static int read_fuse_status(hcmvs_ctx* c, const char* who, const uint32_t* status, uint32_t st[4], const unsigned long long* dWords, unsigned long long* words, int nWords) {
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(st, status, 16, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(words, dWords, (size_t)nWords * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (st[0] != 0) return fail(c, HCMVS_ERR_TIMEOUT, "%s: the settle iteration of a fusion pass gave up; the registered depth maps are left partially fused", who);
	return HCMVS_OK;
}

int hcmvs_filter(hcmvs_ctx* c, uint32_t ref_id, const uint32_t* nbr, int32_t N, int32_t adjust, int32_t n_min_views,
                 int32_t n_min_views_adjust, float depth_diff_threshold, float* out_depth, float* out_conf, uint64_t* n_processed,
                 uint64_t* n_discarded) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!nbr || !out_depth || !out_conf || N < 1 || N > 64) return fail(c, HCMVS_ERR_INVALID, "filter: bad arguments");
	if (N < n_min_views || N < n_min_views_adjust) return fail(c, HCMVS_ERR_INVALID, "filter: depth map %u can not be filtered (%d neighbours)", ref_id, N); // SceneDensify.cpp:3016-3019
	std::vector<DevMap> host;
	int rc = scene_prologue(c, host);
	if (rc) return rc;
	if (ref_id >= host.size() || !host[ref_id].depth) return fail(c, HCMVS_ERR_INVALID, "filter: view %u has no maps", ref_id);
	std::vector<DevMap> nbs((size_t)N);
	for (int n = 0; n < N; ++n) {
		if (nbr[n] >= host.size() || !host[nbr[n]].depth) return fail(c, HCMVS_ERR_INVALID, "filter: neighbour %u has no maps", nbr[n]);
		nbs[n] = host[nbr[n]];
	}
	const DevMap& ref = host[ref_id];
	const size_t area = (size_t)ref.w * ref.h;
	// scratch: keys [N*area u64] | neighbour table | new depth | new conf
	const size_t offNb = area * N * 8, offD = offNb + ((sizeof(DevMap) * N + 255) & ~(size_t)255), offC = offD + area * 4;
	HIPCHK(c, c->fuseScratch.reserve(offC + area * 4, c->stream));
	char* base = c->fuseScratch.get();
	unsigned long long* keys = (unsigned long long*)base;
	DevMap* dNbs = (DevMap*)(base + offNb);
	float* dD = (float*)(base + offD); float* dC = (float*)(base + offC);
	hipStream_t s = c->stream;
	HIPCHK(c, hipMemcpyAsync(dNbs, nbs.data(), sizeof(DevMap) * N, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemsetAsync(c->counters.get(), 0, 64, s));
	launch_fill_u64(keys, ~0ull, area * N, s);
	for (int n = 0; n < N; ++n) launch_filter_splat(ref, nbs[n], keys + area * n, s);
	launch_filter_vote(ref, dNbs, N, keys, adjust, n_min_views, n_min_views_adjust, depth_diff_threshold, dD, dC, c->counters.get<unsigned long long>(), s);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(out_depth, dD, area * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipMemcpyAsync(out_conf, dC, area * 4, hipMemcpyDeviceToHost, s));
	unsigned long long cnt[2] = {0, 0};
	HIPCHK(c, hipMemcpyAsync(cnt, c->counters.get(), 16, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s));
	if (n_processed) *n_processed = cnt[0];
	if (n_discarded) *n_discarded = cnt[1];
	return HCMVS_OK;
}

// Scene::DenseReconstructionFilter (SceneDensify.cpp:4100-4185): the filter stage over the registered maps, batched
int hcmvs_filter_sequence(hcmvs_ctx* c, const uint32_t* ids, int32_t n_ids, int32_t max_neighbors, int32_t adjust, int32_t n_min_views,
                          int32_t n_min_views_adjust, float depth_diff_threshold, hcmvs_filter_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	if (n_ids < 0 || (n_ids > 0 && !ids) || max_neighbors < 1 || max_neighbors > 64) return fail(c, HCMVS_ERR_INVALID, "filter_sequence: bad arguments");
	uint64_t* const imgProc = stats ? stats->image_processed : nullptr;
	uint64_t* const imgDisc = stats ? stats->image_discarded : nullptr;
	if (stats) { memset(stats, 0, sizeof *stats); stats->image_processed = imgProc; stats->image_discarded = imgDisc; }
	for (int i = 0; i < n_ids; ++i) { if (imgProc) imgProc[i] = 0; if (imgDisc) imgDisc[i] = 0; }
	std::vector<DevMap> host;
	int rc = scene_prologue(c, host);
	if (rc) return rc;
	// the images to filter and their neighbours: the first max_neighbors of the list that have maps (SceneDensify.cpp:4116-4131)
	struct Item { int pos; uint32_t id; std::vector<uint32_t> nbs; size_t area; };
	std::vector<Item> items;
	size_t stagePx = 0, nNbAll = 0;
	for (int i = 0; i < n_ids; ++i) {
		if (ids[i] >= host.size() || !host[ids[i]].depth) continue; // :4110-4113
		Item it{i, ids[i], {}, (size_t)host[ids[i]].w * host[ids[i]].h};
		for (uint32_t nb : c->views[ids[i]].neighbors) {
			if (nb >= host.size() || !host[nb].depth) continue;
			it.nbs.push_back(nb);
			if ((int)it.nbs.size() == max_neighbors) break;
		}
		const int N = (int)it.nbs.size();
		if (N < 1 || N < n_min_views || N < n_min_views_adjust) continue; // :3016-3019
		stagePx += it.area; nNbAll += (size_t)N;
		items.push_back(std::move(it));
	}
	if (stats) { stats->n_filtered = (uint32_t)items.size(); stats->n_skipped = (uint32_t)((size_t)n_ids - items.size()); }
	if (items.empty()) return HCMVS_OK;
	hipStream_t s = c->stream;
	size_t cap = 0; // images per batch the environment asks for, 0 = by memory alone
	if (!parse_filter_batch(getenv("HCMVS_FILTER_BATCH"), items.size(), &cap))
		return fail(c, HCMVS_ERR_INVALID, "filter_sequence: HCMVS_FILTER_BATCH='%s' is neither a positive number nor 'all'", getenv("HCMVS_FILTER_BATCH"));
	HIPCHK(c, c->filterStage.reserve(stagePx * 8, s));
	HIPCHK(c, c->filterCnt.reserve(items.size() * 16, s));
	// the batches (filter_plan.h): as many images as their keys fit into half of what is free (the keys buffer a previous call left counts
	// as free).  When the keys cannot be allocated (the reserve has given back the post-filter chain's state by then) the plan is made again
	// with half the bytes, until the largest batch is one image
	std::vector<size_t> need;
	for (const Item& it : items) need.push_back(it.area * it.nbs.size() * 8);
	size_t freeB = 0, totalB = 0;
	HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
	size_t budget = cap ? ~(size_t)0 : (freeB + c->fuseScratch.capacity()) / 2;
	FilterPlan plan;
	for (;;) {
		plan = plan_filter_batches(need, budget, cap);
		const hipError_t e = c->fuseScratch.reserve(plan.keyBytes, s);
		if (e == hipSuccess) break;
		budget = filter_retry_budget(need, plan);
		if (!budget) return fail(c, HCMVS_ERR_HIP, "filter_sequence: no device memory for the z-buffer keys of one image (%zu bytes): %s", plan.keyBytes, hipGetErrorString(e));
	}
	const std::vector<size_t>& first = plan.first;
	const size_t keyBytes = plan.keyBytes;
	const size_t nBatches = first.size() - 1;
	// one table for the whole call: FilterRef per image | the neighbours' DevMaps | pairs | first workgroup per pair and per image, batch
	// after batch.  It lives on the host until the synchronisation at the end (the upload is asynchronous).
	Carve cv;
	const size_t offRefs = cv(items.size() * sizeof(FilterRef)), offNbs = cv(nNbAll * sizeof(DevMap)), offPairs = cv(nNbAll * sizeof(FilterPair)),
	             offPairFirst = cv((nNbAll + nBatches) * sizeof(int)), offRefFirst = cv((items.size() + nBatches) * sizeof(int));
	HIPCHK(c, c->filterTab.reserve(cv.size, s));
	std::vector<char> tab(cv.size, 0);
	char* dTab = c->filterTab.get();
	FilterRef* hRefs = (FilterRef*)(tab.data() + offRefs);
	DevMap* hNbs = (DevMap*)(tab.data() + offNbs);
	FilterPair* hPairs = (FilterPair*)(tab.data() + offPairs);
	int* hPairFirst = (int*)(tab.data() + offPairFirst);
	int* hRefFirst = (int*)(tab.data() + offRefFirst);
	struct Launch { size_t ref0, nRefs, pair0, nPairs, pairFirst0, refFirst0, keyWords; int splatBlocks, voteBlocks; };
	std::vector<Launch> launches;
	size_t nbAt = 0, stageAt = 0, pfAt = 0, rfAt = 0;
	for (size_t b = 0; b < nBatches; ++b) {
		Launch L{first[b], first[b + 1] - first[b], nbAt, 0, pfAt, rfAt, 0, 0, 0};
		size_t keyAt = 0;
		for (size_t k = first[b]; k < first[b + 1]; ++k) {
			const Item& it = items[k];
			FilterRef& r = hRefs[k];
			r.map = host[it.id];
			r.nbs = (const DevMap*)(dTab + offNbs) + nbAt;
			r.nNbs = (int32_t)it.nbs.size();
			r.keys = c->fuseScratch.get<unsigned long long>() + keyAt;
			r.newDepth = c->filterStage.get<float>() + stageAt; r.newConf = r.newDepth + it.area;
			r.counters = c->filterCnt.get<unsigned long long>() + 2 * k;
			stageAt += 2 * it.area;
			hRefFirst[rfAt++] = L.voteBlocks;
			L.voteBlocks += filter_blocks(it.area);
			for (size_t n = 0; n < it.nbs.size(); ++n) {
				hNbs[nbAt] = host[it.nbs[n]];
				hPairs[nbAt] = FilterPair{(int32_t)(k - first[b]), (int32_t)n};
				hPairFirst[pfAt++] = L.splatBlocks;
				L.splatBlocks += filter_blocks((size_t)host[it.nbs[n]].w * host[it.nbs[n]].h);
				++nbAt; ++L.nPairs;
			}
			keyAt += it.area * it.nbs.size();
		}
		hPairFirst[pfAt++] = L.splatBlocks;
		hRefFirst[rfAt++] = L.voteBlocks;
		L.keyWords = keyAt;
		launches.push_back(L);
	}
	std::vector<unsigned long long> cnt(items.size() * 2); // (declared before the guard below: it must outlive the copy into it)
	Event ev[2]; // timing; (declared before the guard too: they go after the stream is idle)
	for (Event& e : ev)
		if (e.ensure() != hipSuccess) return fail(c, HCMVS_ERR_HIP, "filter_sequence: hipEventCreate failed");
	// whichever way the call ends: the stream is idle before the host tables (tab, cnt: source and target of asynchronous copies) go
	struct EndGuard { hipStream_t s; ~EndGuard() { (void)hipStreamSynchronize(s); } } endGuard{s};
	HIPCHK(c, hipMemcpyAsync(dTab, tab.data(), cv.size, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemsetAsync(c->filterCnt.get(), 0, items.size() * 16, s));
	HIPCHK(c, hipEventRecord(ev[0].get(), s));
	const FilterRef* dRefs = (const FilterRef*)(dTab + offRefs);
	for (const Launch& L : launches) {
		launch_fill_u64(c->fuseScratch.get<unsigned long long>(), ~0ull, L.keyWords, s);
		launch_filter_splat_batch(dRefs + L.ref0, (const FilterPair*)(dTab + offPairs) + L.pair0, (const int*)(dTab + offPairFirst) + L.pairFirst0, (int)L.nPairs,
		                          L.splatBlocks, s);
		launch_filter_vote_batch(dRefs + L.ref0, (const int*)(dTab + offRefFirst) + L.refFirst0, (int)L.nRefs, L.voteBlocks, adjust, n_min_views, n_min_views_adjust,
		                         depth_diff_threshold, s);
	}
	launch_filter_commit(dRefs, (int)items.size(), s); // every image was voted from the maps as the call found them; now they change
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(ev[1].get(), s));
	HIPCHK(c, hipMemcpyAsync(cnt.data(), c->filterCnt.get(), items.size() * 16, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s)); // the only wait after the first launch: nothing synchronises between the batches
	if (stats) {
		for (size_t k = 0; k < items.size(); ++k) {
			stats->n_processed += cnt[2 * k]; stats->n_discarded += cnt[2 * k + 1];
			if (imgProc) imgProc[items[k].pos] = cnt[2 * k];
			if (imgDisc) imgDisc[items[k].pos] = cnt[2 * k + 1];
		}
		for (const Launch& L : launches) stats->batch = std::max(stats->batch, (uint32_t)L.nRefs);
		stats->device_bytes = keyBytes + stagePx * 8 + cv.size + items.size() * 16;
		HIPCHK(c, hipEventElapsedTime(&stats->ms_device, ev[0].get(), ev[1].get()));
	}
	return HCMVS_OK;
}

int hcmvs_set_fuse_order(hcmvs_ctx* c, int32_t mode) {
	if (!c) return HCMVS_ERR_INVALID;
	if (mode != 0 && mode != 1) return fail(c, HCMVS_ERR_INVALID, "set_fuse_order: mode %d not in {0, 1}", mode);
	c->fuseOrder = mode;
	return HCMVS_OK;
}

int hcmvs_fuse_cloud(hcmvs_ctx* c, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
                     float normal_diff_deg, float depthweight, float normalweight, hcmvs_cloud* cloud) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!cloud) return fail(c, HCMVS_ERR_INVALID, "fuse: null cloud");
	const uint64_t capacity = cloud->capacity, viewCapacity = cloud->view_ids ? cloud->views_capacity : 0;
	float* xyz = cloud->xyz; float* normal = cloud->normal; uint8_t* bgr = cloud->bgr; uint32_t* n_views = cloud->n_views;
	cloud->n_points = cloud->n_depths = cloud->n_view_entries = 0;
	if (cloud->view_ids && !cloud->view_weights) return fail(c, HCMVS_ERR_INVALID, "fuse: view_ids without view_weights");
	if (!order || n_order < 1) return fail(c, HCMVS_ERR_INVALID, "fuse: bad arguments");
	const auto tCall = std::chrono::steady_clock::now();
	const bool wantCloud = xyz != nullptr; // without xyz only the fusion's side effects (claims, invalidated depths) and counts are produced
	std::vector<DevMap> host;
	int rc = scene_prologue(c, host);
	if (rc) return rc;
	FuseDims dims;
	rc = fuse_call_dims(c, "fuse", plan_maps(c, host), order, n_order, dims);
	if (rc) return rc;
	const size_t maxArea = dims.maxArea;
	const int maxNb = dims.maxNb;
	hipStream_t s = c->stream;
	launch_unclaim(c->dMaps.get<DevMap>(), (int)host.size(), s); // no claim mark may be left over from a fusion that failed half way
	const size_t scanBytes = (fuse_scan_temp_bytes((int)maxArea) + 255) & ~(size_t)255;
	// the device cloud (context scratch) ...
	const FuseCloudOut oc = plan_fuse_cloud_out(capacity, viewCapacity, wantCloud, normal != nullptr, bgr != nullptr, n_views != nullptr);
	HIPCHK(c, c->fuseScratch.reserve(oc.bytes, s));
	char* cb = c->fuseScratch.get();
	float* cX = (float*)(cb + oc.xyz); float* cN = normal ? (float*)(cb + oc.normal) : nullptr; uint8_t* cB = bgr ? (uint8_t*)(cb + oc.bgr) : nullptr;
	uint32_t* cV = n_views || viewCapacity ? (uint32_t*)(cb + oc.nViews) : nullptr;
	uint32_t* cVI = viewCapacity ? (uint32_t*)(cb + oc.viewIds) : nullptr; float* cVW = viewCapacity ? (float*)(cb + oc.viewWeights) : nullptr;
	// ... and the per-pass tables (sized for the largest image)
	const FuseCloudPass o = plan_fuse_cloud_pass(dims, fuse_settle_bytes(maxArea), kCtlBytes, scanBytes, viewCapacity != 0);
	HIPCHK(c, c->passScratch.reserve(o.bytes, s));
	const int vstride = maxNb + 1;
	const float normalError = cosf(fd2r(normal_diff_deg * normalweight)); // SceneDensify.cpp:3310
	const float thDepth = depth_diff_threshold * depthweight;             // SceneDensify.cpp:3400
	const bool debug = getenv("HCMVS_FUSE_DEBUG") != nullptr; // per image: a synchronisation and a line on stderr

	// Every pass of the fusion is enqueued on the context's stream, no host synchronisation between the images (stream order is the
	// order of the sequential loop, SceneDensify.cpp:3302).  What the host would have to know in between stays on the device: the
	// running point / view-entry totals an image's compaction starts from (fuse_advance_kernel), and the word that says a cloud or
	// view-list capacity was exceeded.
	char* b = c->passScratch.get();
	FusePass t(b, o, dims.stride);
	t.thDepth = thDepth; t.normalError = normalError; t.nMinViewsFuse = n_min_views_fuse; t.vstride = vstride;
	unsigned long long* totals = (unsigned long long*)(b + o.totals);
	uint32_t* flag32 = (uint32_t*)(b + o.flag32); uint32_t* pos = (uint32_t*)(b + o.pos);
	float* pxyz = (float*)(b + o.xyz); float* pnrm = (float*)(b + o.nrm); uint8_t* pbgr = (uint8_t*)(b + o.bgr);
	uint32_t* pviews = viewCapacity ? (uint32_t*)(b + o.pviews) : nullptr; float* pweights = viewCapacity ? (float*)(b + o.pweights) : nullptr;
	uint32_t* voff = viewCapacity ? (uint32_t*)(b + o.voff) : nullptr;
	const auto tPasses = std::chrono::steady_clock::now();
	HIPCHK(c, hipMemsetAsync(t.status, 0, 64, s));
	HIPCHK(c, hipMemsetAsync(totals, 0, 64, s));
	for (int oi = 0; oi < n_order; ++oi) {
		const DevMap& A = host[order[oi]];
		const int n = A.w * A.h;
		const auto tPass = std::chrono::steady_clock::now();
		HIPCHK(c, hipMemsetAsync(t.counters, 0, 64, s)); // the counters of this image alone
		rc = enqueue_fuse_pass(c, A, t, pxyz, cN ? pnrm : nullptr, cB ? pbgr : nullptr, pviews, pweights, c->fuseOrder, wantCloud);
		if (rc) return rc;
		if (wantCloud)
			launch_fuse_compact(n, t.flag, flag32, pos, b + o.scan, scanBytes, pxyz, pnrm, pbgr, t.nv, 0, capacity, cX, cN, cB, cV, pviews, pweights, vstride,
			                    voff, 0, viewCapacity, cVI, cVW, totals, s);
		launch_fuse_advance(t.counters, totals, wantCloud ? capacity : 0, wantCloud ? viewCapacity : 0, t.status, s);
		if (debug) {
			unsigned long long cnt[5] = {0, 0, 0, 0, 0};
			uint32_t ctlWords[kCtlBytes / 4];
			HIPCHK(c, hipMemcpyAsync(cnt, t.counters, 40, hipMemcpyDeviceToHost, s));
			HIPCHK(c, hipMemcpyAsync(ctlWords, t.ctl, kCtlBytes, hipMemcpyDeviceToHost, s));
			HIPCHK(c, hipStreamSynchronize(s));
			fprintf(stderr, "fuse: image %u: %u pending pixels, %llu become points; settle iteration: %u steps, work lists", A.id, ctlWords[kCtlPending], cnt[3], ctlWords[kCtlSteps]);
			for (int k = 0; k <= kSettleSteps; ++k) fprintf(stderr, " %u", ctlWords[kCtlWork + k]);
			fprintf(stderr, "; %.0f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tPass).count());
		}
	}
	launch_unclaim(c->dMaps.get<DevMap>(), (int)host.size(), s); // the claim marks come off the depth maps
	uint32_t st[4] = {0, 0, 0, 0};
	unsigned long long tot[3] = {0, 0, 0};
	rc = read_fuse_status(c, "fuse", t.status, st, totals, tot, 3);
	if (rc) return rc;
	if (st[3] == 1) return fail(c, HCMVS_ERR_CAPACITY, "fuse: cloud capacity %llu exceeded", (unsigned long long)capacity);
	if (st[3] == 2) return fail(c, HCMVS_ERR_CAPACITY, "fuse: view-list capacity %llu exceeded", (unsigned long long)viewCapacity);
	const auto tCopy = std::chrono::steady_clock::now();
	const unsigned long long total = tot[0], viewTotal = viewCapacity && wantCloud ? tot[1] : 0;
	if (wantCloud) HIPCHK(c, hipMemcpyAsync(xyz, cX, total * 12, hipMemcpyDeviceToHost, s));
	if (normal) HIPCHK(c, hipMemcpyAsync(normal, cN, total * 12, hipMemcpyDeviceToHost, s));
	if (bgr) HIPCHK(c, hipMemcpyAsync(bgr, cB, total * 3, hipMemcpyDeviceToHost, s));
	if (n_views) HIPCHK(c, hipMemcpyAsync(n_views, cV, total * 4, hipMemcpyDeviceToHost, s));
	if (viewCapacity && wantCloud) {
		HIPCHK(c, hipMemcpyAsync(cloud->view_ids, cVI, viewTotal * 4, hipMemcpyDeviceToHost, s));
		HIPCHK(c, hipMemcpyAsync(cloud->view_weights, cVW, viewTotal * 4, hipMemcpyDeviceToHost, s));
	}
	HIPCHK(c, hipStreamSynchronize(s));
	if (debug) {
		const auto now = std::chrono::steady_clock::now();
		fprintf(stderr, "fuse: %d images, %llu points: setup %.1f ms, passes %.1f ms, copy of the cloud to the host %.1f ms\n", n_order, total,
		        std::chrono::duration<double, std::milli>(tPasses - tCall).count(), std::chrono::duration<double, std::milli>(tCopy - tPasses).count(),
		        std::chrono::duration<double, std::milli>(now - tCopy).count());
	}
	cloud->n_points = total;
	cloud->n_depths = tot[2];
	cloud->n_view_entries = wantCloud ? viewTotal : tot[1]; // a counting call (no xyz) reports what the cloud's view lists would hold
	return HCMVS_OK;
}

int hcmvs_fuse(hcmvs_ctx* c, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
               float normal_diff_deg, float depthweight, float normalweight, uint64_t capacity, float* xyz, float* normal,
               uint8_t* bgr, uint32_t* n_views, uint64_t* n_points, uint64_t* n_depths) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!n_points) return fail(c, HCMVS_ERR_INVALID, "fuse: bad arguments");
	hcmvs_cloud cl;
	memset(&cl, 0, sizeof cl);
	cl.capacity = capacity; cl.xyz = xyz; cl.normal = normal; cl.bgr = bgr; cl.n_views = n_views;
	const int rc = hcmvs_fuse_cloud(c, order, n_order, n_min_views_fuse, depth_diff_threshold, normal_diff_deg, depthweight, normalweight, &cl);
	*n_points = cl.n_points;
	if (n_depths) *n_depths = cl.n_depths;
	return rc;
}

// The post-filter chain with its fusions computed incrementally (pf_kernels.hip): the first fusion of the chain evaluates every pixel,
// each later one only what depends on the estimates that changed since (the pixels the previous image's gap interpolation filled, the
// estimates the previous fusion zeroed).  Same decisions as a fusion from scratch, fusion after fusion.  Returns -1 when the chain can
// not run this way (state does not fit the device, an image occurs twice, too many images) -- the caller then fuses from scratch.
static int postfilter_chain_incremental(hcmvs_ctx* c, const std::vector<DevMap>& host, const std::vector<PlanMap>& maps, size_t maxArea, size_t maxIdArea,
                                        const uint32_t* ids, int32_t n_ids, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
                                        float normal_diff_deg, int32_t gap_size, uint64_t* n_filled) {
	// layout of the state (fuse_plan.h); maxArea: the largest image of the order, maxIdArea: the largest image to filter
	const PfChainPlan lay = plan_pf_chain(maps, ids, n_ids, order, n_order, maxIdArea, sizeof(PfImage), pf_pass_scratch_bytes(maxArea), kCtlBytes);
	if (!lay.ok) return -1;
	const size_t off = lay.bytes, held = c->pfState.capacity();
	if (held < off) {
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return -1;
		if (off > freeB + held || off > (freeB + held) / 10 * 9) { (void)hipGetLastError(); return -1; } // does not fit (with a margin): fuse from scratch
		if (c->pfState.reserve(off, c->stream) != hipSuccess) return -1;
	}
	if (getenv("HCMVS_FUSE_DEBUG")) fprintf(stderr, "postfilter: chain of %d images, fusions computed incrementally (%.1f MB of state kept between them)\n", n_ids, off / 1048576.0);
	// from here on nothing may allocate through the reclaimer: it would free pfState under the pointers below
	char* b = c->pfState.get();
	hipStream_t s = c->stream;
	std::vector<PfImage> pf(host.size());
	memset(pf.data(), 0, pf.size() * sizeof(PfImage));
	for (size_t id = 0; id < host.size(); ++id) {
		const DevMap& m = host[id];
		if (!m.depth) continue;
		const size_t n = (size_t)m.w * m.h;
		const PfImagePlan& L = lay.images[id];
		PfImage& P = pf[id];
		P.own = (uint16_t*)(b + L.own); P.chgNow = (uint8_t*)(b + L.chgNow); P.valNext = (uint8_t*)(b + L.valNext); P.anyChg = (uint32_t*)(b + lay.anyChg) + id;
		HIPCHK(c, hipMemsetAsync(P.own, 0xFF, n * 2, s));
		HIPCHK(c, hipMemsetAsync(P.chgNow, 0, n, s));
		HIPCHK(c, hipMemsetAsync(P.valNext, 0, n, s));
		if (!L.inOrder) continue;
		const size_t nNb = (size_t)std::max(m.nNeighbors, 1);
		P.tgt = (uint32_t*)(b + L.tgt); P.head = (uint32_t*)(b + L.head); P.next = (uint32_t*)(b + L.next); P.acc = (uint8_t*)(b + L.acc);
		P.mm = (uint32_t*)(b + L.mm); P.fm = (uint32_t*)(b + L.fm); P.stamp = (uint32_t*)(b + L.stamp); P.touch = (uint32_t*)(b + L.touch); P.stride = L.stride;
		launch_fill_u32(P.tgt, 0x03FFFFFFu, n * nNb, s); // "projects nowhere", never linked
		HIPCHK(c, hipMemsetAsync(P.head, 0xFF, nNb * L.stride * 4, s));
		HIPCHK(c, hipMemsetAsync(P.acc, 0, n, s));
		HIPCHK(c, hipMemsetAsync(P.mm, 0, n * 4, s)); HIPCHK(c, hipMemsetAsync(P.fm, 0, n * 4, s));
		HIPCHK(c, hipMemsetAsync(P.stamp, 0, n * 4, s)); HIPCHK(c, hipMemsetAsync(P.touch, 0, n * 4, s));
	}
	uint32_t* anyChg = (uint32_t*)(b + lay.anyChg);
	HIPCHK(c, hipMemsetAsync(anyChg, 0, host.size() * 4, s));
	PfImage* dPf = (PfImage*)(b + lay.table);
	HIPCHK(c, hipMemcpyAsync(dPf, pf.data(), pf.size() * sizeof(PfImage), hipMemcpyHostToDevice, s));
	uint32_t* ctl = (uint32_t*)(b + lay.ctl); unsigned long long* counters = (unsigned long long*)(b + lay.counters); uint32_t* status = (uint32_t*)(b + lay.status);
	float* dF = (float*)(b + lay.dF); float* dF2 = (float*)(b + lay.dF2); float* nF = (float*)(b + lay.nF);
	HIPCHK(c, hipMemsetAsync(status, 0, 64, s));
	HIPCHK(c, hipMemsetAsync(counters, 0, 64, s));
	const float normalError = cosf(fd2r(normal_diff_deg)); // plain thresholds (SceneDensify.cpp:2083, 2177)
	for (int k = 0; k < n_ids; ++k) {
		if (k > 0) launch_pf_roll(c->dMaps.get<DevMap>(), dPf, (int)host.size(), anyChg, s);
		for (int oi = 0; oi < n_order; ++oi)
			launch_pf_pass(host[order[oi]], oi, c->dMaps.get<DevMap>(), dPf, pf[order[oi]], k == 0, depth_diff_threshold, normalError, n_min_views_fuse, (uint32_t)k, b + lay.scratch, ctl, status, s);
		View& v = c->views.find(ids[k])->second;
		launch_pf_filter(v.w, v.h, v.mDepth, v.mNormal, v.mConf, pf[ids[k]], v.gra.get<uint8_t>(), dF, dF2, nF, gap_size, depth_diff_threshold * 2.5f, counters + 5, s);
	}
	uint32_t st[4] = {0, 0, 0, 0};
	unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
	const int rc = read_fuse_status(c, "postfilter", status, st, counters, cnt, 6);
	if (rc) return rc;
	if (n_filled) *n_filled = cnt[5];
	return HCMVS_OK;
}

// The post-filters of one outer iteration, image after image.  Every image costs a complete fusion over all maps (that IS the
// fork's RemoveSmallSegments, SceneDensify.cpp:2048-2275), so the fusion here is the one thing that must be cheap: it produces no
// cloud, and all its passes are enqueued on the context's stream WITHOUT host synchronisation -- stream order is the image order
// of the sequential algorithm.  One synchronisation at the end of the sequence.
int hcmvs_postfilter_sequence(hcmvs_ctx* c, const uint32_t* ids, int32_t n_ids, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse,
                              float depth_diff_threshold, float normal_diff_deg, int32_t gap_size, uint64_t* n_filled) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!ids || n_ids < 1 || !order || n_order < 1 || gap_size < 0) return fail(c, HCMVS_ERR_INVALID, "postfilter: bad arguments");
	for (int k = 0; k < n_ids; ++k) {
		auto it = c->views.find(ids[k]);
		if (it == c->views.end() || !it->second.mDepth || !it->second.mNormal) return fail(c, HCMVS_ERR_INVALID, "postfilter: view %u has no registered depth + normal maps", ids[k]);
	}
	std::vector<DevMap> host;
	int rc = scene_prologue(c, host);
	if (rc) return rc;
	const std::vector<PlanMap> maps = plan_maps(c, host);
	FuseDims dims;
	rc = fuse_call_dims(c, "postfilter", maps, order, n_order, dims);
	if (rc) return rc;
	size_t maxIdArea = 0;
	for (int k = 0; k < n_ids; ++k) { View& v = c->views.find(ids[k])->second; maxIdArea = std::max(maxIdArea, (size_t)v.w * v.h); rc = ensure_gradient(c, v); if (rc) return rc; }
	// a chain of two or more images: every fusion after the first is computed incrementally when the state fits the device
	// (HCMVS_PF_FULL=1: every fusion from scratch, the path of rounds 1-3, kept as the fall-back and for comparison)
	if (n_ids >= 2 && !getenv("HCMVS_PF_FULL")) {
		launch_unclaim(c->dMaps.get<DevMap>(), (int)host.size(), c->stream); // no claim mark may be left over from a fusion that failed half way
		rc = postfilter_chain_incremental(c, host, maps, dims.maxArea, maxIdArea, ids, n_ids, order, n_order, n_min_views_fuse, depth_diff_threshold, normal_diff_deg,
		                                  gap_size, n_filled);
		if (rc >= 0) return rc;
	}
	const FusePostfilterPass o = plan_postfilter_pass(dims, fuse_settle_bytes(dims.maxArea), kCtlBytes, maxIdArea);
	HIPCHK(c, c->passScratch.reserve(o.bytes, c->stream));
	char* b = c->passScratch.get();
	FusePass t(b, o, dims.stride);
	t.thDepth = depth_diff_threshold; t.normalError = cosf(fd2r(normal_diff_deg)); // plain thresholds (SceneDensify.cpp:2083, 2177)
	t.nMinViewsFuse = n_min_views_fuse; t.vstride = dims.maxNb + 1;
	float* dF = (float*)(b + o.dF); float* dF2 = (float*)(b + o.dF2); float* nF = (float*)(b + o.nF);
	hipStream_t s = c->stream;
	launch_unclaim(c->dMaps.get<DevMap>(), (int)host.size(), s); // no claim mark may be left over from a fusion or post-filter that failed half way
	HIPCHK(c, hipMemsetAsync(t.status, 0, 64, s));
	HIPCHK(c, hipMemsetAsync(t.counters, 0, 64, s)); // counters[5]: pixels filled, summed over the sequence
	for (int k = 0; k < n_ids; ++k) {
		View& v = c->views.find(ids[k])->second;
		for (int oi = 0; oi < n_order; ++oi) {
			// no point outputs; the fork's RemoveSmallSegments visits the pixels in raster order (SceneDensify.cpp:2130-2131), whatever
			// hcmvs_set_fuse_order says about FuseDepthMaps
			rc = enqueue_fuse_pass(c, host[order[oi]], t, nullptr, nullptr, nullptr, nullptr, nullptr, 0, false);
			if (rc) return rc;
		}
		launch_postfilter(v.w, v.h, v.mDepth, v.mNormal, v.mConf, c->dMaps.get<DevMap>(), (int)host.size(), v.gra.get<uint8_t>(), dF, dF2, nF, gap_size, depth_diff_threshold * 2.5f,
		                  t.counters + 5, s);
	}
	uint32_t st[4] = {0, 0, 0, 0};
	unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
	rc = read_fuse_status(c, "postfilter", t.status, st, t.counters, cnt, 6);
	if (rc == HCMVS_ERR_TIMEOUT) {
		launch_unclaim(c->dMaps.get<DevMap>(), (int)host.size(), s); // an estimate or a saved map must never see a claim mark (negative depth)
		(void)hipStreamSynchronize(s);
	}
	if (rc) return rc;
	if (n_filled) *n_filled = cnt[5];
	return HCMVS_OK;
}

int hcmvs_postfilter(hcmvs_ctx* c, uint32_t id, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
                     float normal_diff_deg, int32_t gap_size, uint64_t* n_filled) {
	return hcmvs_postfilter_sequence(c, &id, 1, order, n_order, n_min_views_fuse, depth_diff_threshold, normal_diff_deg, gap_size, n_filled);
}

int hcmvs_estimate_point_colors(hcmvs_ctx* c, uint64_t n, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids, uint8_t* bgr) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!xyz || !n_views || !view_ids || !bgr) return fail(c, HCMVS_ERR_INVALID, "estimate_point_colors: null argument");
	if (n == 0) return HCMVS_OK;
	std::vector<DevMap> host;
	int rc = scene_prologue(c, host);
	if (rc) return rc;
	std::vector<unsigned long long> off(n + 1, 0);
	for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + n_views[i];
	for (unsigned long long k = 0; k < off[n]; ++k)
		if (!find_view(c, "estimate_point_colors", view_ids[k])) return HCMVS_ERR_INVALID; // (the map table covers every registered view)
	hipStream_t s = c->stream;
	DevBuf dX(c), dOff(c), dV(c), dC(c); // freed on return
	if (dX.reserve(n * 12, s) != hipSuccess || dOff.reserve((n + 1) * 8, s) != hipSuccess || dV.reserve(std::max<unsigned long long>(off[n], 1) * 4, s) != hipSuccess ||
	    dC.reserve(n * 3, s) != hipSuccess) return fail(c, HCMVS_ERR_HIP, "estimate_point_colors: out of device memory");
	HIPCHK(c, hipMemcpyAsync(dX.get(), xyz, n * 12, hipMemcpyHostToDevice, s));
	HIPCHK(c, hipMemcpyAsync(dOff.get(), off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
	if (off[n]) HIPCHK(c, hipMemcpyAsync(dV.get(), view_ids, off[n] * 4, hipMemcpyHostToDevice, s));
	launch_point_colors(n, dX.get<float>(), dOff.get<unsigned long long>(), dV.get<uint32_t>(), c->dMaps.get<DevMap>(), dC.get<uint8_t>(), s);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(bgr, dC.get(), n * 3, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s));
	return HCMVS_OK;
}

int hcmvs_estimate_point_normals(hcmvs_ctx* c, uint64_t n, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids, int32_t k, float* normal) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!xyz || !n_views || !view_ids || !normal || k < 3 || k > 32) return fail(c, HCMVS_ERR_INVALID, "estimate_point_normals: bad arguments (3 <= k <= 32)");
	if (n == 0) return HCMVS_OK;
	// a NaN or an infinite coordinate leaves the bounding box, and with it the grid of the k-nearest search (cell size, dimensions, the
	// levels of the climb), undefined: refused here, before anything reaches the device
	for (uint64_t i = 0; i < n; ++i)
		if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
			return fail(c, HCMVS_ERR_INVALID, "estimate_point_normals: point %llu has a coordinate that is not finite", (unsigned long long)i);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	uint32_t maxId = 0;
	for (auto& kv : c->views) maxId = std::max(maxId, kv.first);
	std::vector<double> centres(3 * ((size_t)maxId + 1), 0.0); // camera centres by view id
	for (auto& kv : c->views) for (int q = 0; q < 3; ++q) centres[3 * (size_t)kv.first + q] = kv.second.C[q];
	std::vector<uint32_t> first(n);
	unsigned long long off = 0;
	for (uint64_t i = 0; i < n; ++i) {
		if (n_views[i] < 1) return fail(c, HCMVS_ERR_INVALID, "estimate_point_normals: point %llu has no view", (unsigned long long)i);
		if (!find_view(c, "estimate_point_normals", view_ids[off])) return HCMVS_ERR_INVALID;
		first[i] = view_ids[off];
		off += n_views[i];
	}
	std::string err;
	DevBuf scratch(c); // freed on return
	const int rc = hcmvs::pca_normals_device(n, xyz, first.data(), centres.data(), (size_t)maxId + 1, k, normal, scratch, c->stream, err);
	if (rc) return fail(c, rc == 1 ? HCMVS_ERR_INVALID : HCMVS_ERR_HIP, "%s", err.c_str());
	return HCMVS_OK;
}

int hcmvs_point_cloud_filter(hcmvs_ctx* c, uint64_t n, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids, uint32_t n_images,
                             const int32_t* wh, const double* K, const double* R, const double* C, int32_t th_remove, int32_t* visibility,
                             uint32_t* kept, uint64_t* n_kept, hcmvs_visibility_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	if (!n_kept || (n && (!xyz || !n_views || !view_ids || !kept)) || (n_images && (!wh || !K || !R || !C)))
		return fail(c, HCMVS_ERR_INVALID, "point_cloud_filter: null argument");
	if (n >= 0xFFFFFFFFull) return fail(c, HCMVS_ERR_INVALID, "point_cloud_filter: 2^32 - 1 points or more");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	std::vector<int32_t> vis(n);
	hcmvs::VisCounters st;
	std::string err;
	DevBuf scratch(c); // freed on return
	const int rc = hcmvs::point_cloud_visibility_device(n, xyz, n_views, view_ids, n_images, wh, K, R, C, vis.data(), st, scratch, c->stream, err);
	if (rc) return fail(c, rc == 1 ? HCMVS_ERR_INVALID : HCMVS_ERR_HIP, "%s", err.c_str());
	// RFOREACH + PointCloud::RemovePoint -> cList::RemoveAt (List.h:1070-1077): the last point moves into the hole.  Position i still holds
	// point i when the loop reaches it, so the permutation is order[i] = order[--size] for every removed i, from the back
	uint64_t size = n;
	for (uint64_t i = 0; i < n; ++i) kept[i] = (uint32_t)i;
	for (uint64_t i = n; i-- > 0;)
		if (vis[i] <= th_remove) kept[i] = kept[--size];
	*n_kept = size;
	if (visibility && n) memcpy(visibility, vis.data(), n * 4);
	if (stats) {
		stats->pairs = st.pairs; stats->skipped_pairs = st.skipped; stats->fallback_pairs = st.fallback; stats->candidates = st.candidates;
		stats->hits = st.hits; stats->device_bytes = st.deviceBytes; stats->ms_device = st.ms;
	}
	return HCMVS_OK;
}

int hcmvs_sample_mesh(hcmvs_ctx* c, uint32_t n_vertices, const float* vertices, uint32_t n_faces, const uint32_t* faces, const float* texcoords,
                      const uint8_t* texture, int32_t tex_w, int32_t tex_h, float sample, uint64_t seed, uint64_t capacity, float* xyz, uint32_t* face_of_point,
                      uint8_t* bgr, uint64_t* n_points, hcmvs_mesh_sample_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	if (n_points) *n_points = 0;
	if (stats) memset(stats, 0, sizeof *stats);
	if (!n_points) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: null argument");
	if (n_faces == 0) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: the mesh has no faces");
	if (!faces || (n_vertices && !vertices)) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: null argument");
	if (n_faces >= 0x7FFFFFFFu) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: 2^31 - 1 faces or more");
	if (!(sample != 0.f) || !(sample > -2147483648.f)) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: sample is %g (a density > 0 or minus a number of points expected)", (double)sample);
	if (texture && !texcoords) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: a texture without texture coordinates");
	if (texcoords && !texture) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: texture coordinates without a texture");
	if (texture && (tex_w <= 0 || tex_h <= 0)) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: texture of %d x %d pixels", tex_w, tex_h);
	// a NaN or an infinite coordinate makes the areas, and with them the counts, undefined: refused here, before anything reaches the device
	for (uint32_t i = 0; i < n_vertices; ++i)
		if (!std::isfinite(vertices[3 * (size_t)i]) || !std::isfinite(vertices[3 * (size_t)i + 1]) || !std::isfinite(vertices[3 * (size_t)i + 2]))
			return fail(c, HCMVS_ERR_INVALID, "sample_mesh: vertex %u has a coordinate that is not finite", i);
	for (uint32_t f = 0; f < n_faces; ++f)
		for (int q = 0; q < 3; ++q)
			if (faces[3 * (size_t)f + q] >= n_vertices)
				return fail(c, HCMVS_ERR_INVALID, "sample_mesh: face %u names vertex %u of %u", f, faces[3 * (size_t)f + q], n_vertices);
	if (texcoords)
		for (uint32_t f = 0; f < n_faces; ++f)
			for (int q = 0; q < 6; ++q)
				if (!std::isfinite(texcoords[6 * (size_t)f + q])) return fail(c, HCMVS_ERR_INVALID, "sample_mesh: face %u has a texture coordinate that is not finite", f);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	hcmvs::MeshSampleInput in;
	in.nVertices = n_vertices; in.nFaces = n_faces; in.vertices = vertices; in.faces = faces; in.texcoords = texcoords; in.texture = texture;
	in.texW = tex_w; in.texH = tex_h; in.sample = sample; in.seed = seed;
	hcmvs::MeshSampleCounters st;
	std::string err;
	const int rc = hcmvs::sample_mesh_device(in, capacity, xyz, face_of_point, bgr, stats != nullptr, st, c, c->stream, err);
	*n_points = st.points;
	if (stats) {
		stats->n_faces = n_faces; stats->n_zero_area_faces = st.zeroAreaFaces; stats->n_points = st.points; stats->area = st.area; stats->density = st.density;
		stats->ms_device = st.ms; stats->device_bytes = st.deviceBytes;
	}
	if (rc) return fail(c, rc == 1 ? HCMVS_ERR_INVALID : HCMVS_ERR_HIP, "%s", err.c_str());
	return HCMVS_OK;
}

void hcmvs_default_view_select_params(hcmvs_view_select_params* p) {
	if (!p) return;
	const hcmvs::ViewSelectParams d; // DepthMap.cpp:72-86, SceneDensify.cpp:313-322
	p->n_min_views = d.nMinViews; p->n_min_point_views = d.nMinPointViews; p->n_max_views = d.nMaxViews; p->number_views = d.numberViews;
	p->optim_angle_deg = d.optimAngleDeg; p->min_angle_deg = d.minAngleDeg; p->max_angle_deg = d.maxAngleDeg; p->min_area = d.minArea;
	p->min_scale = d.minScale; p->max_scale = d.maxScale; p->min_score_ratio = d.minScoreRatio; p->min_score = d.minScore;
}

int hcmvs_select_views(hcmvs_ctx* c, uint32_t n_images, const int32_t* wh, const double* K, const double* R, const double* C, uint64_t n, const float* xyz,
                       const uint32_t* n_views, const uint32_t* view_ids, const hcmvs_view_select_params* params, const hcmvs_view_selection* o,
                       hcmvs_view_select_stats* stats) {
	if (!c) return HCMVS_ERR_INVALID;
	if (stats) memset(stats, 0, sizeof *stats);
	if (!params || !o || (n_images && (!wh || !K || !R || !C)) || (n && (!xyz || !n_views || !view_ids)))
		return fail(c, HCMVS_ERR_INVALID, "select_views: null argument");
	if (!o->status || !o->n_seen || !o->avg_depth || !o->n_candidates || !o->n_neighbors || !o->n_srcs || !o->nb_id || !o->nb_points || !o->nb_scale ||
	    !o->nb_angle || !o->nb_area || !o->nb_score || !o->src_scale)
		return fail(c, HCMVS_ERR_INVALID, "select_views: null output array");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	hcmvs::ViewSelectInput in;
	in.nImages = n_images; in.wh = wh; in.K = K; in.R = R; in.C = C; in.nPoints = n; in.xyz = xyz; in.nViews = n_views; in.viewIds = view_ids;
	hcmvs::ViewSelectParams p;
	p.nMinViews = params->n_min_views; p.nMinPointViews = params->n_min_point_views; p.nMaxViews = params->n_max_views; p.numberViews = params->number_views;
	p.optimAngleDeg = params->optim_angle_deg; p.minAngleDeg = params->min_angle_deg; p.maxAngleDeg = params->max_angle_deg; p.minArea = params->min_area;
	p.minScale = params->min_scale; p.maxScale = params->max_scale; p.minScoreRatio = params->min_score_ratio; p.minScore = params->min_score;
	hcmvs::ViewSelectOutput out;
	out.status = o->status; out.nSeen = o->n_seen; out.avgDepth = o->avg_depth; out.nCandidates = o->n_candidates; out.nNeighbors = o->n_neighbors;
	out.nSrcs = o->n_srcs; out.nbId = o->nb_id; out.nbPoints = o->nb_points; out.nbScale = o->nb_scale; out.nbAngle = o->nb_angle; out.nbArea = o->nb_area;
	out.nbScore = o->nb_score; out.srcScale = o->src_scale; out.pointsFirst = (unsigned long long*)o->points_first; out.pointIds = o->point_ids;
	hcmvs::ViewSelectCounters st;
	std::string err;
	const int rc = hcmvs::select_views_device(in, p, out, st, c, c->stream, err);
	if (stats) { stats->pairs = st.pairs; stats->skipped = st.skipped; stats->chunks = st.chunks; stats->device_bytes = st.deviceBytes; stats->ms_device = st.ms; }
	if (rc) return fail(c, rc == 1 ? HCMVS_ERR_INVALID : HCMVS_ERR_HIP, "%s", err.c_str());
	return HCMVS_OK;
}

#ifdef HCMVS_STAMPS
// diagnostic build only: per-phase cycle totals of the sweep workers (not part of the public header)
int hcmvs_debug_stamps(hcmvs_ctx* c, unsigned long long* out, int reset) {
	if (!c || !out) return HCMVS_ERR_INVALID;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	hcmvs::debug_read_stamps(out, reset);
	return HCMVS_OK;
}
#endif

} // extern "C"
