// C face of hc-mvs_amd/host/driver_plan.h for tests/test_driver_plan.py (ctypes).  Links nothing of the library and nothing of HIP.
// Results of variable length come back as text: "key=value" lines, lists separated by blanks.
#include "../hc-mvs_amd/host/driver_plan.h"
#include "../include/hcmvs_hip.h"

#include <cstdio>

using namespace driverplan;
typedef unsigned long long u64;

static std::string g_text; // what the last text-returning call said (the caller copies it before the next call)

template <typename T>
static std::string list_of(const std::vector<T>& v) {
	std::ostringstream s;
	for (size_t i = 0; i < v.size(); ++i) s << (i ? " " : "") << v[i];
	return s.str();
}
static std::string f32(float v) { char b[40]; snprintf(b, sizeof b, "%.9g", (double)v); return b; }

// a scene's images as the plans see them: sizes, validity, neighbour ids nbIds[nbFirst[i] .. nbFirst[i + 1]) and source views likewise
static std::vector<PlanImage> images_of(int n, const int* w, const int* h, const int* valid, const int* nbFirst, const uint32_t* nbIds, const int* srcFirst, const uint32_t* srcIds) {
	std::vector<PlanImage> images((size_t)n);
	for (int i = 0; i < n; ++i) {
		PlanImage& im = images[(size_t)i];
		im.id = (uint32_t)i; im.w = w[i]; im.h = h[i]; im.valid = valid[i] != 0;
		for (int k = nbFirst[i]; k < nbFirst[i + 1]; ++k) im.neighbors.push_back(PlanImage::Nb{nbIds[k], 0, 1.f, 0.f, 0.f, 0.f});
		for (int k = srcFirst[i]; k < srcFirst[i + 1]; ++k) { im.srcs.push_back(srcIds[k]); im.srcScale.push_back(1.f); }
	}
	return images;
}
#define SCENE_PARAMS int n, const int* w, const int* h, const int* valid, const int* nbFirst, const uint32_t* nbIds, const int* srcFirst, const uint32_t* srcIds
#define SCENE_ARGS n, w, h, valid, nbFirst, nbIds, srcFirst, srcIds

extern "C" {

int dp_max_batch() { return HCMVS_MAX_BATCH; }
int dp_known_options(int k, const char** name) {
	const int n = (int)(sizeof kKnownOptions / sizeof kKnownOptions[0]);
	if (k >= 0 && k < n) *name = kKnownOptions[k];
	return n;
}

// parse_options on argv[0 .. argc): every field of Options, "result" and "err"
const char* dp_parse(int argc, char** argv) {
	Options o;
	std::string err;
	const int rc = (int)parse_options(argc, argv, o, err);
	std::ostringstream s;
	s << "result=" << rc << "\nerr=" << err << "\ninput=" << o.input << "\noutput=" << o.output << "\nworkdir=" << o.workdir << "\nignoreMaskLabel=" << o.ignoreMaskLabel
	  << "\nresolutionLevel=" << o.resolutionLevel << "\nnumberViews=" << o.numberViews << "\nnumberViewsFuse=" << o.numberViewsFuse << "\nfusionMode=" << o.fusionMode
	  << "\nverbosity=" << o.verbosity << "\nestimationIters=" << o.estimationIters << "\nestimationItersExternal=" << o.estimationItersExternal
	  << "\nadaptHalfWin=" << o.adaptHalfWin << "\npropagateHalfWin=" << o.propagateHalfWin << "\npropagateStep=" << o.propagateStep
	  << "\nphotometricFlow=" << f32(o.photometricFlow) << "\ndepthweight=" << f32(o.depthweight) << "\nnormalweight=" << f32(o.normalweight)
	  << "\ninitTriangulate=" << o.initTriangulate << "\nminViewsTrustPoint=" << o.minViewsTrustPoint << "\nfuseCount=" << o.fuseCount << "\nfuseOrder=" << o.fuseOrder
	  << "\nestimateColors=" << o.estimateColors << "\nestimateNormals=" << o.estimateNormals << "\nmaxResolution=" << o.maxResolution << "\nminResolution=" << o.minResolution
	  << "\nnOptimize=" << o.nOptimize << "\npostFilter=" << o.postFilter << "\nviewspread=" << o.viewspread << "\npostFilterInterleave=" << o.postFilterInterleave
	  << "\nnFilter=" << o.nFilter << "\nresume=" << o.resume << "\nrestoreHypothesis=" << o.restoreHypothesis << "\ndevice=" << o.device << "\nbatch=" << o.batch
	  << "\ndevices=" << list_of(o.devices) << "\nseed=" << o.seed << "\nthFilterPointCloud=" << o.thFilterPointCloud << "\nsampleMesh=" << f32(o.sampleMesh)
	  << "\nsampleSeed=" << o.sampleSeed << "\nnNotes=" << o.notes.size() << "\n";
	for (const auto& note : o.notes) s << "note=" << note << "\n";
	g_text = s.str();
	return g_text.c_str();
}

// plan_iteration: bit 0 filtered, 1 serial, 2 meet, 3 snapshotSpread, 4 liveSpread, 5 workerSubmitsFinal, 6 mainSubmitsFinal
int dp_iteration(int postFilter, int interleave, int viewspread, int nFilter, int iters, int it, int anyWork) {
	Options o;
	o.postFilter = postFilter; o.postFilterInterleave = interleave; o.viewspread = viewspread; o.nFilter = nFilter; o.estimationItersExternal = iters;
	const IterPlan p = plan_iteration(o, it, anyWork != 0);
	return (p.filtered ? 1 : 0) | (p.serial ? 2 : 0) | (p.meet ? 4 : 0) | (p.snapshotSpread ? 8 : 0) | (p.liveSpread ? 16 : 0) | (p.workerSubmitsFinal ? 32 : 0) |
	       (p.mainSubmitsFinal ? 64 : 0);
}
int dp_stage_submits_final(int nFilter) { Options o; o.nFilter = nFilter; return stage_submits_final(o) ? 1 : 0; }

// plan_deal: fuseOrder[nTodo], dev[n], needGray[nDev * n]
void dp_deal(SCENE_PARAMS, const uint32_t* todo, int nTodo, int nDev, uint32_t* fuseOrder, int* dev, int* needGray) {
	const std::vector<PlanImage> images = images_of(SCENE_ARGS);
	const Deal deal = plan_deal(images, std::vector<uint32_t>(todo, todo + nTodo), nDev);
	for (int k = 0; k < nTodo; ++k) fuseOrder[k] = deal.fuseOrder[(size_t)k];
	for (int i = 0; i < n; ++i) dev[i] = deal.dev[(size_t)i];
	for (int d = 0; d < nDev; ++d) for (int i = 0; i < n; ++i) needGray[d * n + i] = deal.needGray[(size_t)d][(size_t)i];
}
int dp_registered_neighbors(SCENE_PARAMS, uint32_t id, const uint32_t* todo, int nTodo, uint32_t* out) {
	const std::vector<PlanImage> images = images_of(SCENE_ARGS);
	const std::vector<uint32_t> nb = registered_neighbors(images[id], std::vector<uint32_t>(todo, todo + nTodo));
	for (size_t k = 0; k < nb.size(); ++k) out[k] = nb[k];
	return (int)nb.size();
}
// plan_device_budget of device d (after plan_deal): out = resident, perImage, batch, fits, ownImages, needed
void dp_budget(SCENE_PARAMS, const uint32_t* todo, int nTodo, int nDev, int d, u64 freeBytes, int restore, int nFilter, int fusionMode, int fuseCount, int batch, u64* out) {
	const std::vector<PlanImage> images = images_of(SCENE_ARGS);
	const std::vector<uint32_t> td(todo, todo + nTodo);
	const Deal deal = plan_deal(images, td, nDev);
	Options o;
	o.restoreHypothesis = restore; o.nFilter = nFilter; o.fusionMode = fusionMode; o.fuseCount = fuseCount; o.batch = batch;
	const DeviceBudget b = plan_device_budget(images, td, deal, d, (size_t)freeBytes, o);
	out[0] = b.resident; out[1] = b.perImage; out[2] = (u64)b.batch; out[3] = b.fits ? 1 : 0; out[4] = b.ownImages; out[5] = b.needed();
}
// plan_batches: work of device d is workIds[workFirst[d] .. workFirst[d + 1]); "dev: ids" per line
const char* dp_batches(SCENE_PARAMS, int nDev, const int* workFirst, const uint32_t* workIds, int batch) {
	const std::vector<PlanImage> images = images_of(SCENE_ARGS);
	std::vector<std::vector<uint32_t>> work((size_t)nDev);
	for (int d = 0; d < nDev; ++d) work[(size_t)d].assign(workIds + workFirst[d], workIds + workFirst[d + 1]);
	std::ostringstream s;
	for (const Batch& b : plan_batches(images, work, batch)) s << b.dev << ": " << list_of(b.ids) << "\n";
	g_text = s.str();
	return g_text.c_str();
}
void dp_cloud_worst_case(SCENE_PARAMS, const uint32_t* todo, int nTodo, int numberViewsFuse, u64* out) {
	const CloudSize c = cloud_worst_case(images_of(SCENE_ARGS), std::vector<uint32_t>(todo, todo + nTodo), numberViewsFuse);
	out[0] = c.capacity; out[1] = c.viewCapacity;
}
int dp_fusion_counts_first(u64 capacity, u64 viewCapacity, int fuseCount) {
	CloudSize c;
	c.capacity = capacity; c.viewCapacity = viewCapacity;
	return fusion_counts_first(c, fuseCount) ? 1 : 0;
}
int dp_budget_counts_first(u64 allPx, int fuseCount) { return budget_counts_first((size_t)allPx, fuseCount) ? 1 : 0; }
u64 dp_budget_cloud_bytes(u64 allPx, int fuseCount) { return budget_cloud_bytes((size_t)allPx, fuseCount); }

void dp_working_size(int w, int h, unsigned level, unsigned minSize, unsigned maxSize, int* nw, int* nh) { sceneio::working_size(w, h, level, minSize, maxSize, *nw, *nh); }

// image_camera + select_views for every image of a scene with one camera (K at cw x ch, R = I, C = 0) and one pose per image, the images at
// w x h; vertex v is seen by viewIds[viewFirst[v] .. viewFirst[v + 1]).  Per image a line
// "id selected nPoints | srcs | srcScale | neighbour ids | neighbour scales"
const char* dp_select_views(int n, int cw, int ch, const double* K, const double* poseR, const double* poseC, int w, int h, int nVerts, const float* X, const int* viewFirst,
                            const uint32_t* viewIds, int nMaxViews, int numberViews) {
	sceneio::MvsCamera cam;
	cam.w = (uint32_t)cw; cam.h = (uint32_t)ch;
	memcpy(cam.K, K, sizeof cam.K);
	const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	memcpy(cam.R, eye, sizeof eye);
	cam.C[0] = cam.C[1] = cam.C[2] = 0;
	std::vector<PlanImage> images((size_t)n);
	for (int i = 0; i < n; ++i) {
		sceneio::MvsPose q;
		memcpy(q.R, poseR + 9 * i, sizeof q.R); memcpy(q.C, poseC + 3 * i, sizeof q.C);
		PlanImage& im = images[(size_t)i];
		im.id = (uint32_t)i; im.w = w; im.h = h; im.valid = true;
		image_camera(cam, q, w, h, im.cam);
	}
	std::vector<Vertex> verts((size_t)nVerts);
	for (int v = 0; v < nVerts; ++v) {
		memcpy(verts[(size_t)v].X, X + 3 * v, 12);
		for (int k = viewFirst[v]; k < viewFirst[v + 1]; ++k) verts[(size_t)v].views.emplace_back(viewIds[k], 1.f);
	}
	std::ostringstream s;
	for (int i = 0; i < n; ++i) {
		const bool ok = select_views(images, verts, (uint32_t)i, nMaxViews, numberViews);
		const PlanImage& im = images[(size_t)i];
		std::vector<uint32_t> nbIds;
		std::vector<std::string> scl, nbScl;
		for (float v : im.srcScale) scl.push_back(f32(v));
		for (const auto& nb : im.neighbors) { nbIds.push_back(nb.id); nbScl.push_back(f32(nb.scale)); }
		s << i << " " << (ok ? 1 : 0) << " " << im.points.size() << " | " << list_of(im.srcs) << " | " << list_of(scl) << " | " << list_of(nbIds) << " | " << list_of(nbScl) << "\n";
	}
	g_text = s.str();
	return g_text.c_str();
}

} // extern "C"
