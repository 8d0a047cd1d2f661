/*
 * hc-mvs_amd/host/DensifyPointCloud.cpp -- command-line driver with the reference's DensifyPointCloud interface
 * (frame_main/apps/DensifyPointCloud/DensifyPointCloud.cpp:71-198, 373-449) on top of the C-ABI of
 * include/hcmvs_hip.h.  It reads an `.mvs` scene (MVSI v5, Interface.h:363-619) and the images it names, selects the
 * source views of every image the way Scene::SelectNeighborViews / FilterNeighborViews / InitViews do
 * (Scene.cpp:545-678, SceneDensify.cpp:336-397), runs the PatchMatch estimate for the requested outer iterations
 * (Scene::DenseReconstruction, SceneDensify.cpp:3532-3574, 3684), writes raw 'DR' depth maps
 * (DepthMap.cpp:2781-2846), fuses them (SceneDensify.cpp:3265-3495) and saves `<out>.ply` + `<out>.mvs`
 * (DensifyPointCloud.cpp:447-449).  With --filter-point-cloud < 0 it only filters the cloud of the input scene by visibility
 * (Scene::PointCloudFilter, DensifyPointCloud.cpp:399-414) and saves `<out>_filtered.mvs` + `.ply`.  With --sample-mesh != 0 the input is a
 * PLY triangle mesh: a point cloud is sampled on it (Mesh::SamplePoints, DensifyPointCloud.cpp:384-398) and saved as `<out>.ply`.
 *
 * Deliberately narrower than the reference ("defined subset"): images are read from binary
 * PPM/PGM files (no PNG/JPEG codecs here); the initial maps come from the Delaunay triangulation of the sparse points
 * (--n-initTriangulate 1, the default), from the previous run's maps under <working-folder>/depthmap + normalmap
 * (--n-initTriangulate 0, the fork's hand-off, SceneDensify.cpp:527-553) or from a splat (--min-views-trust-point 1); --n-nOptimize
 * gates the fork's post-filters (RemoveSmallSegments + GapInterpolation) as in the reference; --n-viewspread 1 lets every pixel also try
 * the estimates of its source views' own maps from outer iteration 1 on (DepthMap.cpp:1504-1608; default 0 here, 1 in the reference, so
 * that existing command lines keep their results; one device); --plane-priors 1 generates depth priors from planes fitted inside the
 * label 255 of seman/<stem>.quad.pgm|ppm on outer iteration n - 2 (--export-priors <dir> writes them; --plane-clusters 1 keeps the largest
 * connected component of a plane's inliers, on cells of --ransac-cluster average spacings; --plane-refit n refits the winning plane of
 * every round by n least-squares steps);
 * --geo-consistency 1 blends every view score with a reprojection term against the source views' maps of the previous outer iteration
 * (fed by --n-para_tapa, --n-para_tapa2, --n-txthreshold, --n-txthreshold2, --n-photo2geo, --geo-max-px; one device; D14);
 * optical flow, --use-semantic, --n-usegeoconsistency and SGM modes are not available and the corresponding flags are accepted and ignored with a note.
 *
 * How the run is laid out in time (the reference overlaps image k + 1's InitViews with image k's estimate, SceneDensify.cpp:3699-3703;
 * here the unit is a batch of reference images):
 *   load     all cores decode / resize the images and select the source views at the same time; uploads go out as images arrive
 *   estimate a loader thread prepares the initial maps of batch k + 1 (triangulation on all cores, upload) while the device
 *            estimates batch k; after the last outer iteration a copier thread brings finished batches back and a pool of writer
 *            threads saves the depth maps while the next batch is estimated and while the fusion runs
 *   resume   an image whose final depth map is already in the working folder is not estimated again (SceneDensify.cpp:3865-3880)
 *
 * Where what is: driver_plan.h decides (options, view selection, dealing, memory budget, batches, the schedule of an outer iteration, cloud
 * sizes; no HIP), scene_io.h reads and writes the files; this file owns the device objects and the threads (Loader, Saver, Workers) and runs
 * the phases of main() in their order.
 */
#include "../../include/hcmvs_hip.h"
#include "driver_plan.h"
#include "ply_mesh.h"
#include "scene_io.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

using namespace sceneio;
using namespace driverplan;

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

namespace {

// One batch of reference images whose initial maps the loader thread prepares while the device works on the batch before it
// (the reference requests "next image initialization to be performed while computing this depth-map", SceneDensify.cpp:3699-3703)
struct Prepared { bool ready = false; int failed = 0; uint32_t failedId = 0; };

// the initial maps of one image (SceneDensify.cpp:772-812) and, for the `restore` variant, its hint maps: host part
struct InitMaps { std::vector<float> d, n, hd, hn; int failed = 0; };

// the final maps of one image on the host, on their way to the files (Saver)
struct SaveJob { uint32_t id; std::vector<float> d, n, c; };

// host -> device through two page-locked buffers on a stream of its own: memcpy into one half while the other is on its way
struct Uploader {
	static constexpr size_t kPiece = (size_t)32 << 20;
	hipStream_t s = nullptr; char* pin = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; int k = 0;
	bool init() {
		if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return false;
		if (hipHostMalloc((void**)&pin, 2 * kPiece, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pin = nullptr; }
		for (auto& e : ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
		return true;
	}
	bool copy(void* dst, const void* src, size_t bytes) {
		if (!pin) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
		for (size_t off = 0; off < bytes; off += kPiece, k ^= 1) {
			const size_t n = std::min(kPiece, bytes - off);
			if (used[k] && hipEventSynchronize(ev[k]) != hipSuccess) return false;
			memcpy(pin + (size_t)k * kPiece, (const char*)src + off, n);
			if (hipMemcpyAsync((char*)dst + off, pin + (size_t)k * kPiece, n, hipMemcpyHostToDevice, s) != hipSuccess || hipEventRecord(ev[k], s) != hipSuccess) return false;
			used[k] = true;
		}
		return true;
	}
	bool drain() { return hipStreamSynchronize(s) == hipSuccess; }
	~Uploader() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } if (pin) (void)hipHostFree(pin); for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
};
// --filter-point-cloud < 0 (DensifyPointCloud.cpp:399-414): Scene::Load, Scene::PointCloudFilter(th) on the first device of --devices,
// then <output base>_filtered.mvs / .ply; no densify runs.  The cameras are taken at their own resolution and no image is opened, except
// the header of an image whose camera has no resolution (Scene::LoadInterface reads the size from the image then).
int run_point_cloud_filter(const Options& o) {
	const int th = o.thFilterPointCloud;
	const double tStart = now_s();
	std::vector<MvsPlatform> platforms; std::vector<MvsImage> mimages; std::vector<Vertex> verts;
	std::vector<float> normals; std::vector<uint8_t> colors;
	if (!load_mvs(o.input, platforms, mimages, verts, &normals, &colors)) { fprintf(stderr, "error: can not load '%s'\n", o.input.c_str()); return EXIT_FAILURE; }
	if (verts.empty()) { fprintf(stderr, "error: empty initial point-cloud\n"); return EXIT_FAILURE; }
	const size_t n = verts.size(), m = mimages.size();
	std::vector<int32_t> wh(2 * std::max<size_t>(m, 1), 0);
	std::vector<double> K(9 * std::max<size_t>(m, 1), 0.0), R(9 * std::max<size_t>(m, 1), 0.0), C(3 * std::max<size_t>(m, 1), 0.0);
	for (size_t i = 0; i < m; ++i) {
		const MvsImage& mi = mimages[i];
		if (mi.poseID == 0xFFFFFFFFu || mi.platformID >= platforms.size()) continue; // uncalibrated: its pairs are skipped
		const MvsPlatform& p = platforms[mi.platformID];
		if (mi.cameraID >= p.cams.size() || mi.poseID >= p.poses.size()) continue;
		const MvsCamera& c = p.cams[mi.cameraID];
		int w = (int)c.w, h = (int)c.h;
		if (!w || !h) {
			const std::string path = mi.name[0] == '/' ? mi.name : dirname_of(o.input) + "/" + mi.name;
			if (!pnm_size(path, w, h)) { fprintf(stderr, "error: failed loading image '%s' (binary PPM/PGM expected)\n", path.c_str()); return EXIT_FAILURE; }
		}
		Camera cam;
		image_camera(c, p.poses[mi.poseID], w, h, cam);
		wh[2 * i] = w; wh[2 * i + 1] = h;
		memcpy(&K[9 * i], cam.K, 72); memcpy(&R[9 * i], cam.R, 72); memcpy(&C[3 * i], cam.C, 24);
	}
	std::vector<float> xyz(3 * n);
	std::vector<uint32_t> nv(n), ids;
	std::vector<float> wts;
	std::vector<size_t> first(n + 1, 0);
	for (size_t i = 0; i < n; ++i) {
		memcpy(&xyz[3 * i], verts[i].X, 12);
		nv[i] = (uint32_t)verts[i].views.size();
		first[i + 1] = first[i] + nv[i];
		for (const auto& v : verts[i].views) { ids.push_back(v.first); wts.push_back(v.second); }
	}
	if (ids.empty()) ids.push_back(0);
	hcmvs_ctx* ctx = nullptr;
	if (hcmvs_create(o.devices[0], &ctx) != HCMVS_OK) { fprintf(stderr, "error: device %d is not a usable MI355X (there is no CPU path)\n", o.devices[0]); return EXIT_FAILURE; }
	std::vector<int32_t> vis(n);
	std::vector<uint32_t> kept(n);
	uint64_t nKept = 0;
	hcmvs_visibility_stats st;
	if (hcmvs_point_cloud_filter(ctx, n, xyz.data(), nv.data(), ids.data(), (uint32_t)m, wh.data(), K.data(), R.data(), C.data(), th, vis.data(), kept.data(),
	                             &nKept, &st) != HCMVS_OK) {
		fprintf(stderr, "error: point-cloud filter failed: %s\n", hcmvs_last_error(ctx));
		hcmvs_destroy(ctx);
		return EXIT_FAILURE;
	}
	hcmvs_destroy(ctx);
	const bool hasN = normals.size() == 3 * n, hasC = colors.size() == 3 * n; // RemovePoint moves what exists (PointCloud.cpp:54-69)
	if (o.verbosity > 2) {
		// the histogram of the non-positive visibilities and the removed points, reverse index order (SceneDensify.cpp:4284-4308)
		std::vector<unsigned> counts;
		for (int32_t v : vis) {
			if (v > 0) continue;
			if (counts.size() <= (size_t)-(int64_t)v) counts.resize((size_t)-(int64_t)v + 1, 0);
			++counts[(size_t)-(int64_t)v];
		}
		printf("Visibility lengths (%zu points):", n);
		for (size_t c = 0; c < counts.size(); ++c)
			if (counts[c]) printf("\n\t%3zu - %9u", c, counts[c]);
		printf("\n");
		size_t nOut = 0;
		for (int32_t v : vis) nOut += v <= th;
		RawArray<float> ox(3 * nOut), on(0);
		RawArray<uint8_t> oc(hasC ? 3 * nOut : 0);
		size_t k = 0;
		for (size_t i = n; i-- > 0;)
			if (vis[i] <= th) {
				memcpy(ox.data() + 3 * k, &xyz[3 * i], 12);
				if (hasC) memcpy(oc.data() + 3 * k, &colors[3 * i], 3);
				++k;
			}
		const std::string outliers = o.workdir + "/scene_dense_outliers.ply";
		if (!save_ply(outliers, ox, on, oc)) { fprintf(stderr, "error: can not write '%s'\n", outliers.c_str()); return EXIT_FAILURE; }
		printf("Point visibility checks: %llu pairs (%llu skipped: unknown or uncalibrated image), %llu exact-path pairs, %.1f candidates per pair, "
		       "%llu votes, %.1f MiB device memory, %.2f ms device time\n", (unsigned long long)st.pairs, (unsigned long long)st.skipped_pairs,
		       (unsigned long long)st.fallback_pairs, st.pairs ? (double)st.candidates / (double)st.pairs : 0.0, (unsigned long long)st.hits,
		       st.device_bytes / 1048576.0, st.ms_device);
	}
	// the kept cloud in the reference's order; views, weights, normals and colours move with their point
	size_t nEntries = 0;
	for (uint64_t k = 0; k < nKept; ++k) nEntries += nv[kept[k]];
	RawArray<float> kx(3 * nKept), kn(hasN ? 3 * nKept : 0), kw(nEntries);
	RawArray<uint8_t> kc(hasC ? 3 * nKept : 0);
	RawArray<uint32_t> knv(nKept), kids(nEntries);
	size_t e = 0;
	for (uint64_t k = 0; k < nKept; ++k) {
		const size_t i = kept[k];
		memcpy(kx.data() + 3 * k, &xyz[3 * i], 12);
		if (hasN) memcpy(kn.data() + 3 * k, &normals[3 * i], 12);
		if (hasC) memcpy(kc.data() + 3 * k, &colors[3 * i], 3);
		knv.data()[k] = nv[i];
		for (size_t v = first[i]; v < first[i + 1]; ++v, ++e) { kids.data()[e] = ids[v]; kw.data()[e] = wts[v]; }
	}
	const std::string base = o.output.substr(0, o.output.rfind('.')) + "_filtered";
	if (!save_mvs(base + ".mvs", platforms, mimages, kx, kn, kc, knv, kids, kw)) { fprintf(stderr, "error: can not write '%s.mvs'\n", base.c_str()); return EXIT_FAILURE; }
	if (!save_ply(base + ".ply", kx, kn, kc)) { fprintf(stderr, "error: can not write '%s.ply'\n", base.c_str()); return EXIT_FAILURE; }
	if (o.verbosity > 1)
		printf("Point-cloud filtered: %llu/%zu points (%d%%) (%.2f s)\n", (unsigned long long)nKept, n, (int)std::lround(100.0 * (double)nKept / (double)n), now_s() - tStart);
	return EXIT_SUCCESS;
}

// --sample-mesh != 0 (DensifyPointCloud.cpp:384-398): Mesh::Load, Mesh::SamplePoints on the first device of --devices, then <output base>.ply;
// nothing else runs.  > 0: points per square unit, < 0: minus the number of points.  The input is a PLY triangle mesh (host/ply_mesh.h); the
// draws are the counter-based ones of DESIGN.md section 5 (D11) under --seed.  Colours when the mesh has texture coordinates and its
// "comment TextureFile" names a binary PPM.
int run_sample_mesh(const Options& o) {
	const float sample = o.sampleMesh;
	const unsigned long long seed = o.sampleSeed;
	const size_t dot = o.input.rfind('.');
	std::string ext = dot == std::string::npos ? std::string() : o.input.substr(dot);
	for (char& ch : ext) ch = (char)tolower((unsigned char)ch);
	if (ext == ".obj") { fprintf(stderr, "error: --sample-mesh reads PLY meshes only: OBJ input '%s' is not supported\n", o.input.c_str()); return EXIT_FAILURE; }
	plymesh::Mesh mesh;
	std::string err;
	if (!plymesh::load(o.input, mesh, err)) { fprintf(stderr, "error: can not load the mesh '%s': %s\n", o.input.c_str(), err.c_str()); return EXIT_FAILURE; }
	const size_t nV = mesh.vertices.size() / 3, nF = mesh.faces.size() / 3;
	if (nF == 0) { fprintf(stderr, "error: the mesh '%s' has no faces\n", o.input.c_str()); return EXIT_FAILURE; }
	std::vector<uint8_t> tex;
	int tw = 0, th = 0;
	bool textured = false;
	if (mesh.texcoords.size() == 6 * nF && !mesh.textureFile.empty()) {
		const std::string path = mesh.textureFile[0] == '/' ? mesh.textureFile : dirname_of(o.input) + "/" + mesh.textureFile;
		textured = load_pnm(path, tw, th, tex) && tw > 0 && th > 0;
		if (!textured && o.verbosity > 1) fprintf(stderr, "note: the texture '%s' is not a readable binary PPM: positions only\n", path.c_str());
	} else if (o.verbosity > 1 && (!mesh.texcoords.empty() || !mesh.textureFile.empty()))
		fprintf(stderr, "note: the mesh has %s: positions only\n", mesh.texcoords.empty() ? "a texture but no texture coordinates" : "texture coordinates but no texture");
	hcmvs_ctx* ctx = nullptr;
	if (hcmvs_create(o.devices[0], &ctx) != HCMVS_OK) { fprintf(stderr, "error: device %d is not a usable MI355X (there is no CPU path)\n", o.devices[0]); return EXIT_FAILURE; }
	const double t0 = now_s();
	const float* tc = textured ? mesh.texcoords.data() : nullptr;
	const uint8_t* tx = textured ? tex.data() : nullptr;
	uint64_t n = 0;
	hcmvs_mesh_sample_stats st;
	auto bail = [&](const char* what) {
		fprintf(stderr, "error: %s: %s\n", what, hcmvs_last_error(ctx));
		hcmvs_destroy(ctx);
		return EXIT_FAILURE;
	};
	// counted first, so that the host buffers are exactly as large as the cloud
	if (hcmvs_sample_mesh(ctx, (uint32_t)nV, mesh.vertices.data(), (uint32_t)nF, mesh.faces.data(), tc, tx, tw, th, sample, seed, 0, nullptr, nullptr, nullptr, &n, &st) != HCMVS_OK)
		return bail("sampling the mesh failed");
	RawArray<float> xyz(3 * n), nrm(0);
	RawArray<uint8_t> bgr(textured ? 3 * n : 0);
	if (xyz.size() != 3 * n || (textured && bgr.size() != 3 * n)) { fprintf(stderr, "error: out of host memory for %llu points\n", (unsigned long long)n); hcmvs_destroy(ctx); return EXIT_FAILURE; }
	if (n && hcmvs_sample_mesh(ctx, (uint32_t)nV, mesh.vertices.data(), (uint32_t)nF, mesh.faces.data(), tc, tx, tw, th, sample, seed, n, xyz.data(), nullptr,
	                           textured ? bgr.data() : nullptr, &n, &st) != HCMVS_OK)
		return bail("sampling the mesh failed");
	hcmvs_destroy(ctx);
	if (o.verbosity > 0) printf("Sample mesh completed: %llu points (%.0f ms)\n", (unsigned long long)n, (now_s() - t0) * 1e3);
	if (o.verbosity > 2)
		printf("Mesh sampling: %zu faces (%llu of zero area), area %g, density %g, %.1f MiB device memory, %.2f ms device time\n", nF,
		       (unsigned long long)st.n_zero_area_faces, st.area, st.density, st.device_bytes / 1048576.0, st.ms_device);
	const std::string base = o.output.substr(0, o.output.rfind('.'));
	if (!save_ply(base + ".ply", xyz, nrm, bgr)) { fprintf(stderr, "error: can not write '%s.ply'\n", base.c_str()); return EXIT_FAILURE; }
	return EXIT_SUCCESS;
}

// ---- a densify run: what it works on -------------------------------------------------------------------------------------------------
// (the phases below return false after they have said what went wrong; main() turns that into EXIT_FAILURE)
#define CHK(call) do { const int rc_ = (call); if (rc_ != HCMVS_OK) { fprintf(stderr, "error: %s -> %d (%s)\n", #call, rc_, hcmvs_last_error(ctx)); return false; } } while (0)
#define HIPOK(call) do { if ((call) != hipSuccess) { fprintf(stderr, "error: %s failed\n", #call); return false; } } while (0)

struct ImageData : PlanImage {
	std::vector<uint32_t> srcImages;            // the scene images behind srcs
	float dMin = 0, dMax = 0;
	int dev = 0;                                                    // index of the device context that estimates this image (--devices)
	float *dDepth = nullptr, *dNormal = nullptr, *dConf = nullptr; // device maps, on the owner's device
	float *gDepth = nullptr, *gNormal = nullptr, *gConf = nullptr; // the copy on the first device, where the post-filters and the fusion run (== d* when dev == 0)
	float *dHintDepth = nullptr, *dHintNormal = nullptr;            // previous level's maps, resized (restore variant)
	std::vector<float> prior;                                       // --depth-priors: the image's prior depth map (w * h), empty: none; --plane-priors 1: the
	                                                                // generated one, filled on outer iteration n - 2
	bool hasRegion = false;                                         // --plane-priors 1: a label file was found and its region registered
	// what a depth-map file says about its image: scene image ids, not the ids of resampled copies
	DmapImage file_header() const { return DmapImage{name, id, w, h, cam.K, cam.R, cam.C, srcImages.empty() ? srcs : srcImages, dMin, dMax}; }
};

// One context and one host thread per entry of --devices; devs[0] is where the post-filters and the fusion run.
struct DeviceCtx { int ordinal = 0; hcmvs_ctx* ctx = nullptr; int createRc = HCMVS_OK; std::mutex upMu; std::vector<uint32_t> work; };

struct JoinedThread { std::thread t; ~JoinedThread() { if (t.joinable()) t.join(); } };
struct StreamGuard { hipStream_t s = nullptr; ~StreamGuard() { if (s) (void)hipStreamDestroy(s); } };
// --n-viewspread (one device): what the source views offer.  Batch schedule: before every outer iteration >= 1 the maps of all images are
// copied into a second buffer set (20 B per pixel of the scene) -- every estimate of the iteration reads its source views as the previous
// iteration left them, post-filters included.  Interleaved schedule: the live maps (the reference's order; an image is never its own
// source view, and one image is estimated per call).
struct SpreadSnap { float *d = nullptr, *n = nullptr, *c = nullptr; };
struct SpreadSnaps {
	std::map<uint32_t, SpreadSnap> m;
	~SpreadSnaps() { for (auto& kv : m) for (float* q : {kv.second.d, kv.second.n, kv.second.c}) if (q) (void)hipFree(q); }
};

struct Loader;
struct Saver;
struct Workers;

struct Run {
	Run(const Options& opts, double t0);
	~Run();
	const double tStart;
	Options o;                             // (the memory budget may lower o.batch)
	std::vector<DeviceCtx> devs;
	const int nDev;
	hcmvs_ctx* ctx = nullptr;              // the context of the post-filters and the fusion: devs[0].ctx
	std::vector<MvsPlatform> platforms; std::vector<MvsImage> mimages; std::vector<Vertex> verts;
	std::vector<ImageData> images;
	std::vector<std::string> paths;
	unsigned nValid = 0;
	std::vector<char> selected;            // per image: the view selection found source views
	std::vector<uint32_t> todo, work;      // the images that get maps; the ones of them that are estimated (not resumed), in todo order
	Deal deal;                             // fusion order, device of every image, gray images per device
	std::vector<Batch> batches;
	hcmvs_params prm;
	std::mutex errMu; std::string loadError;
	double tLoaded = 0, tInit = 0, tPostfilter = 0, tEstimated = 0, tCopied = 0;
	std::mutex speckleMu; hcmvs_speckle_stats speckle = {}; // --speckle-size: the counters of the run, summed over its calls (one per batch and device)
	// threads and device objects, destroyed in the reverse order: the workers stop first, the context creation is joined last
	JoinedThread creator;
	std::unique_ptr<Loader> loader;
	std::unique_ptr<Saver> saver;
	StreamGuard xs;                        // the stream of the exchange between the devices and of the view-spread copies
	SpreadSnaps spreadSnap;
	std::unique_ptr<Workers> workers;
};

// ---- the loader: initial maps of batch k + 1 while batch k is estimated (outer iteration 0) ----
//   nMinViewsTrustPoint < 2      splat of the sparse points (SceneDensify.cpp:783-808)
//   initTriangulate != 0         Delaunay triangulation of the sparse points (DepthMapsData::InitDepthMap, DepthMap.cpp:1796-1936)
//   initTriangulate == 0         the previous run's maps, <working-folder>/depthmap/depth%04u.dmap + normalmap/normal%04u.dmap
//                                (what run.sh moves between the stages; SceneDensify.cpp:527-553), else <working-folder>/depth%04u.dmap
// restore-hypothesis: the previous level's maps, enlarged with INTER_AREA, are the extra last-sweep hypothesis and widen the
// depth range (restore/libs/MVS/SceneDensify.cpp:508-532)
struct Loader {
	Run& r;
	std::vector<Prepared> prepared;
	std::mutex mu; std::condition_variable cv;
	std::string error;
	std::thread t;
	explicit Loader(Run& run) : r(run), prepared(run.batches.size()), t(&Loader::serve, this) {}
	~Loader() { if (t.joinable()) t.join(); }
	void join() { t.join(); }
	// batch b has its initial maps on its device; false (and the reason on stderr) when that failed
	bool wait(size_t b) {
		const Options& o = r.o;
		std::unique_lock<std::mutex> g(mu);
		cv.wait(g, [&] { return prepared[b].ready || !error.empty(); });
		if (!error.empty()) { fprintf(stderr, "error: %s\n", error.c_str()); return false; }
		const Prepared& pr = prepared[b];
		if (pr.failed == 2) { fprintf(stderr, "error: can not read the previous level's maps of image %u ('%s/depthmap/depth%04u.dmap' + normalmap, or '%s/depth%04u.dmap')\n", pr.failedId, o.workdir.c_str(), pr.failedId, o.workdir.c_str(), pr.failedId); return false; }
		if (pr.failed == 3) { fprintf(stderr, "error: the previous level's depth map of image %u holds no valid depth\n", pr.failedId); return false; }
		if (pr.failed) { fprintf(stderr, "error: initialisation of image %u failed (%s)\n", pr.failedId, pr.failed == 4 ? "device memory" : "no sparse point in front of the image"); return false; }
		return true;
	}

private:
	void fail(const char* what) { std::lock_guard<std::mutex> g(mu); error = what; cv.notify_all(); }
	bool previous_maps(uint32_t id, DmapFile& out) const {
		const std::string& dir = r.o.workdir;
		DmapFile dm, nm;
		if (load_dmap(map_path(dir, "/depthmap/depth%04u.dmap", id), dm, 1) && load_dmap(map_path(dir, "/normalmap/normal%04u.dmap", id), nm, 2) &&
		    dm.w == nm.w && dm.h == nm.h) {
			out.w = dm.w; out.h = dm.h; out.d.swap(dm.d); out.n.swap(nm.n);
			return true;
		}
		return load_dmap(map_path(dir, "/depth%04u.dmap", id), out, 3);
	}
	// the previous run's maps as the initial maps of `im`, with the depth range they span
	void hand_over(ImageData& im, InitMaps& M) const {
		const size_t n = im.pixels();
		DmapFile pm;
		if (!previous_maps(im.id, pm)) { M.failed = 2; return; }
		if (r.o.verbosity > 2) printf("read  :  %s (%dx%d -> %dx%d)\n", map_path(r.o.workdir, "/depthmap/depth%04u.dmap", im.id).c_str(), pm.w, pm.h, im.w, im.h);
		// the reference hands maps over between runs of the SAME level (run.sh: restore at level l, then frame_main at level l)
		// and uses them as they are (its INTER_CUBIC resize is to the map's own size, SceneDensify.cpp:541-542); maps of
		// another size are brought to this one with that cubic kernel
		if (pm.w == im.w && pm.h == im.h) { M.d.swap(pm.d); M.n.swap(pm.n); }
		else { resize_cubic(pm.d, pm.w, pm.h, 1, M.d, im.w, im.h); resize_cubic(pm.n, pm.w, pm.h, 3, M.n, im.w, im.h); }
		// depth range of the map, SceneDensify.cpp:544-553: over EVERY value of the handed-over map, the empty pixels (0) included
		// -- an estimated map always has them (its border), so the lower bound is 0, exactly what the `restore` branch below ends
		// up with (one rule for both; DESIGN.md section 5, D7: the reference's running min / max start from uninitialised members).
		// Values the cubic kernel pushed below 0 next to holes (maps of another size only) count as empty.
		float lo = 3.402823466e+38f, hi = 0.f;
		for (size_t q_ = 0; q_ < n; ++q_) {
			if (!(M.d[q_] > 0.f)) M.d[q_] = 0.f;
			lo = std::min(lo, M.d[q_]); hi = std::max(hi, M.d[q_]);
			if (M.d[q_] == 0.f) continue;
			float* q = &M.n[3 * q_];
			const float len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
			if (len > 0.f) { q[0] /= len; q[1] /= len; q[2] /= len; }
		}
		if (!(hi > 0.f)) { M.failed = 3; return; }
		im.dMin = lo * 0.9f; im.dMax = hi * 1.1f;
	}
	// the `restore` variant's hint maps of `im`
	void restore_hint(ImageData& im, InitMaps& M) const {
		const size_t n = im.pixels();
		DmapFile pm;
		if (!previous_maps(im.id, pm) || pm.w > im.w || pm.h > im.h) { M.failed = 2; return; }
		M.hd.resize(n); M.hn.resize(3 * n);
		// cv::resize(..., INTER_AREA) to the current size (restore/libs/MVS/SceneDensify.cpp:523-524)
		if (hcmvs_resize_area_up(pm.d.data(), pm.w, pm.h, 1, M.hd.data(), im.w, im.h) != HCMVS_OK ||
		    hcmvs_resize_area_up(pm.n.data(), pm.w, pm.h, 3, M.hn.data(), im.w, im.h) != HCMVS_OK) { M.failed = 2; return; }
		// ... and the depth range takes the enlarged map in, every pixel of it (restore/libs/MVS/SceneDensify.cpp:526-532).  The
		// border rows and columns of an estimated map hold no depth, so the lower bound becomes 0 there as it does in the
		// reference; where the coarser level has no estimate there is no extra hypothesis
		float lo = im.dMin, hi = im.dMax;
		for (size_t q_ = 0; q_ < n; ++q_) {
			float& hd = M.hd[q_];
			lo = lo > hd ? hd : lo; hi = hi > hd ? hi : hd;
			float* q = &M.hn[3 * q_];
			const float len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
			if (!(hd > 0.f) || !(len > 0.f)) { hd = 0.f; continue; }
			q[0] /= len; q[1] /= len; q[2] /= len; // the mix of two unit normals is shorter than 1
		}
		im.dMin = std::max(lo, 0.f); im.dMax = hi;
	}
	// the initial maps of one image, on the host
	void init_maps(ImageData& im, InitMaps& M) const {
		const Options& o = r.o;
		const size_t n = im.pixels();
		std::vector<float> pts;
		for (uint32_t idx : im.points) { pts.push_back(r.verts[idx].X[0]); pts.push_back(r.verts[idx].X[1]); pts.push_back(r.verts[idx].X[2]); }
		M.d.assign(n, 0.f); M.n.assign(3 * n, 0.f);
		if (o.minViewsTrustPoint < 2) {
			// the context-free form: the loader's workers never touch the context (it is not thread-safe, and the main thread is
			// registering views meanwhile)
			if (hcmvs_splat_points(im.w, im.h, im.cam.K, im.cam.R, im.cam.C, pts.data(), (int32_t)im.points.size(), M.d.data(), M.n.data(), &im.dMin, &im.dMax) != HCMVS_OK) M.failed = 1;
		} else if (o.initTriangulate || o.restoreHypothesis) { // the `restore` binary always triangulates (restore/libs/MVS/SceneDensify.cpp:508-511)
			if (hcmvs_triangulate_points(im.w, im.h, im.cam.K, im.cam.R, im.cam.C, pts.data(), (int32_t)im.points.size(), 0.f, 1, M.d.data(), M.n.data(),
			                             &im.dMin, &im.dMax) != HCMVS_OK) M.failed = 1;
		} else {
			hand_over(im, M);
			if (M.failed) return;
		}
		if (o.restoreHypothesis && !M.failed) restore_hint(im, M);
	}
	// device memory for the maps of a batch, and the maps into it
	Prepared upload(const std::vector<uint32_t>& ids, const std::vector<InitMaps>& maps, Uploader& up) const {
		Prepared res;
		for (size_t k = 0; k < ids.size() && !res.failed; ++k) if (maps[k].failed) { res.failed = maps[k].failed; res.failedId = ids[k]; }
		for (size_t k = 0; k < ids.size() && !res.failed; ++k) {
			ImageData& im = r.images[ids[k]];
			const size_t n = im.pixels();
			bool ok = hipMalloc(&im.dDepth, n * 4) == hipSuccess && hipMalloc(&im.dNormal, n * 12) == hipSuccess && hipMalloc(&im.dConf, n * 4) == hipSuccess &&
			          up.copy(im.dDepth, maps[k].d.data(), n * 4) && up.copy(im.dNormal, maps[k].n.data(), n * 12) && hipMemsetAsync(im.dConf, 0, n * 4, up.s) == hipSuccess;
			if (ok && r.o.restoreHypothesis)
				ok = hipMalloc(&im.dHintDepth, n * 4) == hipSuccess && hipMalloc(&im.dHintNormal, n * 12) == hipSuccess &&
				     up.copy(im.dHintDepth, maps[k].hd.data(), n * 4) && up.copy(im.dHintNormal, maps[k].hn.data(), n * 12);
			if (!ok) { res.failed = 4; res.failedId = ids[k]; }
		}
		if (!res.failed && !up.drain()) { res.failed = 4; res.failedId = ids.empty() ? 0 : ids[0]; }
		res.ready = true;
		return res;
	}
	void serve() {
		// page-locked staging, one copy stream per device: a pageable hipMemcpy of the initial maps (33 MB per 1080p image) crawls
		std::vector<std::unique_ptr<Uploader>> ups((size_t)r.nDev);
		for (int d = 0; d < r.nDev; ++d) {
			ups[(size_t)d].reset(new Uploader);
			if (hipSetDevice(r.devs[(size_t)d].ordinal) != hipSuccess || !ups[(size_t)d]->init()) { fail("no copy stream for the loader"); return; }
		}
		for (size_t b = 0; b < r.batches.size(); ++b) {
			const std::vector<uint32_t>& ids = r.batches[b].ids;
			if (hipSetDevice(r.devs[(size_t)r.batches[b].dev].ordinal) != hipSuccess) { fail("hipSetDevice failed in the loader"); return; }
			std::vector<InitMaps> maps(ids.size());
#pragma omp parallel for schedule(dynamic, 1)
			for (long k = 0; k < (long)ids.size(); ++k) init_maps(r.images[ids[(size_t)k]], maps[(size_t)k]);
			const Prepared res = upload(ids, maps, *ups[(size_t)r.batches[b].dev]);
			{
				std::lock_guard<std::mutex> g(mu);
				prepared[b] = res;
			}
			cv.notify_all();
			if (res.failed) return;
		}
	}
};

// ---- the saver: copies + files of the final maps, behind the estimation ----
// A copier thread brings the maps of finished batches to the host (its own stream; the device keeps estimating), writer threads put them
// on disk.  The fusion mutates the depth maps (SceneDensify.cpp:3447-3449), so it waits for the copies -- not for the files.
struct Saver {
	static constexpr size_t kMaxQueuedBytes = (size_t)12 << 30; // host memory the copier may run ahead of the writers
	Run& r;
	std::mutex mu; std::condition_variable cv;
	std::deque<uint32_t> toCopy; std::deque<std::unique_ptr<SaveJob>> toWrite;
	size_t bytesQueued = 0, copied = 0, written = 0, submitted = 0;
	bool closing = false; std::string error;
	std::thread copier; std::vector<std::thread> writers;
	explicit Saver(Run& run) : r(run), copier(&Saver::copy_maps, this) { for (int k = 0; k < 4; ++k) writers.emplace_back(&Saver::write_files, this); }
	~Saver() {
		{ std::lock_guard<std::mutex> g(mu); closing = true; if (error.empty() && copied != submitted) error = "aborted"; }
		cv.notify_all();
		if (copier.joinable()) copier.join();
		for (auto& t : writers) if (t.joinable()) t.join();
	}
	// final maps of these images: off to the host, then to the files
	void submit(const std::vector<uint32_t>& ids) {
		std::lock_guard<std::mutex> g(mu);
		for (uint32_t id : ids) { toCopy.push_back(id); ++submitted; }
		cv.notify_all();
	}
	void close() { { std::lock_guard<std::mutex> g(mu); closing = true; } cv.notify_all(); }
	bool wait_copied() { return wait_for(copied); }
	bool wait_written() { return wait_for(written); }

private:
	bool wait_for(const size_t& done) {
		std::unique_lock<std::mutex> g(mu);
		cv.wait(g, [&] { return done == submitted || !error.empty(); });
		if (!error.empty()) { fprintf(stderr, "error: %s\n", error.c_str()); return false; }
		return true;
	}
	void fail(const char* what) { std::lock_guard<std::mutex> g(mu); error = what; cv.notify_all(); }
	bool save_files(const SaveJob& j) const {
		const DmapImage im = r.images[j.id].file_header();
		const std::string& dir = r.o.workdir;
		// depth%04u.dmap: the complete DepthData (what the fusion stage of the reference loads, SceneDensify.cpp:3292); depthmap/ +
		// normalmap/: the hand-off pair the next stage of run.sh picks up (DepthMap.h:76-80, SceneDensify.cpp:3984-3988; raw 'DR'
		// content instead of the reference's boost archive)
		return save_dmap(map_path(dir, "/depth%04u.dmap", j.id), im, j.d.data(), j.n.data(), j.c.data()) &&
		       save_dmap(map_path(dir, "/depthmap/depth%04u.dmap", j.id), im, j.d.data(), nullptr, nullptr) &&
		       save_dmap(map_path(dir, "/normalmap/normal%04u.dmap", j.id), im, nullptr, j.n.data(), nullptr);
	}
	// the next image to copy, once the writers have made room for it; false: nothing more to do
	bool next_to_copy(uint32_t& id) {
		std::unique_lock<std::mutex> g(mu);
		cv.wait(g, [&] { return !toCopy.empty() || closing || !error.empty(); });
		if (!error.empty() || (toCopy.empty() && closing)) return false;
		id = toCopy.front(); toCopy.pop_front();
		const size_t need = r.images[id].pixels() * 20;
		cv.wait(g, [&] { return bytesQueued + need <= kMaxQueuedBytes || toWrite.empty() || !error.empty(); });
		if (!error.empty()) return false;
		bytesQueued += need;
		return true;
	}
	void copy_maps() {
		std::vector<hipStream_t> css((size_t)r.nDev, nullptr); // a map is copied on a stream of the device that holds it
		for (int d = 0; d < r.nDev; ++d)
			if (hipSetDevice(r.devs[(size_t)d].ordinal) != hipSuccess || hipStreamCreateWithFlags(&css[(size_t)d], hipStreamNonBlocking) != hipSuccess) { fail("no copy stream"); return; }
		for (uint32_t id; next_to_copy(id);) {
			const ImageData& im = r.images[id];
			const size_t n = im.pixels();
			std::unique_ptr<SaveJob> j(new SaveJob);
			j->id = id; j->d.resize(n); j->n.resize(3 * n); j->c.resize(n);
			hipStream_t cs = css[(size_t)im.dev];
			const bool ok = hipSetDevice(r.devs[(size_t)im.dev].ordinal) == hipSuccess &&
			                hipMemcpyAsync(j->d.data(), im.dDepth, n * 4, hipMemcpyDeviceToHost, cs) == hipSuccess &&
			                hipMemcpyAsync(j->n.data(), im.dNormal, n * 12, hipMemcpyDeviceToHost, cs) == hipSuccess &&
			                hipMemcpyAsync(j->c.data(), im.dConf, n * 4, hipMemcpyDeviceToHost, cs) == hipSuccess && hipStreamSynchronize(cs) == hipSuccess;
			std::lock_guard<std::mutex> g(mu);
			if (!ok) error = "copy of a depth map to the host failed";
			else { toWrite.push_back(std::move(j)); ++copied; }
			cv.notify_all();
		}
		for (int d = 0; d < r.nDev; ++d) if (css[(size_t)d]) { (void)hipSetDevice(r.devs[(size_t)d].ordinal); (void)hipStreamDestroy(css[(size_t)d]); }
	}
	void write_files() {
		for (;;) {
			std::unique_ptr<SaveJob> j;
			{
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return !toWrite.empty() || (closing && copied == submitted) || !error.empty(); });
				if (toWrite.empty()) break;
				j = std::move(toWrite.front()); toWrite.pop_front();
			}
			const bool ok = save_files(*j);
			std::lock_guard<std::mutex> g(mu);
			bytesQueued -= r.images[j->id].pixels() * 20;
			++written;
			if (!ok && error.empty()) error = "can not write '" + map_path(r.o.workdir, "/depth%04u.dmap", j->id) + "'";
			cv.notify_all();
		}
	}
};

// --plane-priors 1: the prior of `im` from its live maps (ordered behind its estimate on the context's stream), into im.prior -- where
// --depth-priors would have put the file's -- and, with --export-priors, into the file a later run can read
bool generate_plane_prior(Run& r, hcmvs_ctx* dctx, ImageData& im, const hcmvs_batch_item& itx, std::string& err) {
	hcmvs_plane_prior_params pp;
	hcmvs_default_plane_prior_params(&pp);
	pp = plane_prior_params(r.o, pp);
	float* dPrior = nullptr;
	if (hipMalloc(&dPrior, im.pixels() * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); err = "out of device memory for a plane prior"; return false; }
	hcmvs_plane_prior_stats st;
	im.prior.resize(im.pixels());
	const bool ok = hcmvs_generate_plane_prior_device(dctx, im.id, (const float*)itx.d_depth, (const float*)itx.d_normal, (const float*)itx.d_conf, &pp, dPrior, nullptr,
	                                                  nullptr, &st) == HCMVS_OK &&
	                hipMemcpy(im.prior.data(), dPrior, im.pixels() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
	(void)hipFree(dPrior);
	if (!ok) { err = std::string("generating the plane prior of image ") + std::to_string(im.id) + " failed (" + hcmvs_last_error(dctx) + ")"; return false; }
	if (r.o.verbosity > 2)
		printf("Plane prior of image %3u: %d planes from %llu samples (%llu in the fitting set), %llu prior pixels, %.1f ms\n", im.id, st.planes,
		       (unsigned long long)st.samples, (unsigned long long)st.fitting_samples, (unsigned long long)st.prior_pixels, st.ms_device);
	if (r.o.verbosity > 1 && pp.cluster_mul > 0.f)
		printf("Plane clusters of image %3u: %d planes, %d rounds rejected, %llu inliers left (cell %g)\n", im.id, st.planes, st.cluster_rejects,
		       (unsigned long long)st.cluster_left, (double)st.cluster_eps);
	if (r.o.verbosity > 1 && pp.refit_iters > 0) {
		hcmvs_plane_prior_refit_stats rs = {0, 0};
		(void)hcmvs_get_plane_prior_refit_stats(dctx, &rs);
		printf("Plane refit of image %3u: %d of %d rounds refitted, %d steps kept\n", im.id, rs.refit_rounds, st.rounds, rs.refit_steps);
	}
	if (!r.o.exportPriors.empty()) {
		DmapImage hd = im.file_header();
		if (!save_dmap(export_prior_path(r.o, im.id), hd, im.prior.data(), nullptr, nullptr)) { err = "can not write '" + export_prior_path(r.o, im.id) + "'"; return false; }
	}
	return true;
}

// ---- what the workers and the main thread both do ------------------------------------------------------------------------------------
// one launch set for the reference images `ids` (all of device context d)
bool estimate_images(Run& r, int d, const std::vector<uint32_t>& ids, const hcmvs_params& pr, std::string& err) {
	hcmvs_ctx* dctx = r.devs[(size_t)d].ctx;
	std::vector<hcmvs_batch_item> items;
	for (uint32_t id : ids) {
		ImageData& im = r.images[id];
		hcmvs_batch_item itx;
		itx.ref_id = im.id; itx.src_ids = im.srcs.data(); itx.n_src = (int32_t)im.srcs.size(); itx.seed_offset = im.id;
		itx.d_min = im.dMin; itx.d_max = im.dMax; itx.d_depth = im.dDepth; itx.d_normal = im.dNormal; itx.d_conf = im.dConf;
		itx.d_hint_depth = im.dHintDepth; itx.d_hint_normal = im.dHintNormal;
		items.push_back(itx);
	}
	hcmvs_stats st;
	if (hcmvs_estimate_batch_device(dctx, items.data(), (int32_t)items.size(), &pr) != HCMVS_OK || hcmvs_get_stats(dctx, &st) != HCMVS_OK) {
		err = std::string("depth-map estimation failed (") + hcmvs_last_error(dctx) + ")";
		return false;
	}
	// --depth-priors: after the ordinary estimate of outer iteration n - 2 the priors of these images are registered (they stay for the last
	// iteration) and the reference's two extra sweeps run, with the sweep indices n_estimation_iters and + 1 (SceneDensify.cpp:983-1031)
	if (prior_sweeps_after(r.o, pr.it_external)) {
		std::vector<hcmvs_batch_item> extra;
		for (const auto& itx : items) {
			ImageData& im = r.images[itx.ref_id];
			if (r.o.planePriors && im.hasRegion && !generate_plane_prior(r, dctx, im, itx, err)) return false;
			if (im.prior.empty()) continue;
			if (hcmvs_set_depth_prior(dctx, im.id, im.prior.data()) != HCMVS_OK) { err = std::string("registering the depth prior failed (") + hcmvs_last_error(dctx) + ")"; return false; }
			extra.push_back(itx);
		}
		if (!extra.empty() && hcmvs_estimate_sweeps_batch_device(dctx, extra.data(), (int32_t)extra.size(), &pr, pr.n_estimation_iters, 2) != HCMVS_OK) {
			err = std::string("the extra sweeps with the depth priors failed (") + hcmvs_last_error(dctx) + ")";
			return false;
		}
	}
	// --speckle-size: these are the finished maps of the batch (the end pass of the last outer iteration has run): small segments go, before
	// anything reads the maps -- the saver, the post-filters of this iteration, --n-filter, the fusion
	if (r.o.speckleSize > 0 && pr.it_external == r.o.estimationItersExternal - 1) {
		std::vector<hcmvs_speckle_item> sp;
		for (const auto& itx : items) sp.push_back({r.images[itx.ref_id].w, r.images[itx.ref_id].h, itx.d_depth, itx.d_normal, itx.d_conf, nullptr});
		hcmvs_speckle_stats ss;
		if (hcmvs_remove_speckles_batch_device(dctx, sp.data(), (int32_t)sp.size(), r.o.speckleDiff, (uint32_t)r.o.speckleSize, &ss) != HCMVS_OK) {
			err = std::string("the speckle filter failed (") + hcmvs_last_error(dctx) + ")";
			return false;
		}
		std::lock_guard<std::mutex> g(r.speckleMu);
		r.speckle.n_valid += ss.n_valid; r.speckle.n_removed += ss.n_removed; r.speckle.n_segments += ss.n_segments; r.speckle.n_small += ss.n_small;
		r.speckle.largest = std::max(r.speckle.largest, ss.largest); r.speckle.ms_device += ss.ms_device;
	}
	if (r.o.verbosity > 2)
		for (const auto& itx : items)
			printf("Depth-map for image %3u estimated using %2d images: %dx%d (outer iteration %d, batch %.0f ms%s)\n", itx.ref_id,
			       itx.n_src, r.images[itx.ref_id].w, r.images[itx.ref_id].h, pr.it_external, st.ms_total, r.nDev > 1 ? (", device context " + std::to_string(d)).c_str() : "");
	return true;
}
// what the source views offer to view spread: a snapshot of every map (batch schedule) or the live maps (interleaved schedule)
bool offer_spread_maps(Run& r, bool live, std::string& err) {
	hcmvs_ctx* ctx = r.ctx;
	hipStream_t xs = r.xs.s;
	if (hcmvs_synchronize(ctx) != HCMVS_OK) { err = hcmvs_last_error(ctx); return false; }
	for (uint32_t id : r.todo) {
		ImageData& im = r.images[id];
		if (!im.dDepth || !im.dNormal || !im.dConf) continue;
		const size_t n = im.pixels();
		const float *sd = im.dDepth, *sn = im.dNormal, *sc = im.dConf;
		if (!live) {
			SpreadSnap& sp = r.spreadSnap.m[id];
			if (!sp.d && (hipMalloc(&sp.d, n * 4) != hipSuccess || hipMalloc(&sp.n, n * 12) != hipSuccess || hipMalloc(&sp.c, n * 4) != hipSuccess)) { err = "no device memory for the view-spread copy of the depth maps (20 B per pixel of the scene)"; return false; }
			if (hipMemcpyAsync(sp.d, im.dDepth, n * 4, hipMemcpyDeviceToDevice, xs) != hipSuccess || hipMemcpyAsync(sp.n, im.dNormal, n * 12, hipMemcpyDeviceToDevice, xs) != hipSuccess ||
			    hipMemcpyAsync(sp.c, im.dConf, n * 4, hipMemcpyDeviceToDevice, xs) != hipSuccess) { err = "copying the depth maps for view spread failed"; return false; }
			sd = sp.d; sn = sp.n; sc = sp.c;
		}
		if (hcmvs_set_spread_maps_device(ctx, id, sd, sn, sc) != HCMVS_OK) { err = hcmvs_last_error(ctx); return false; }
	}
	if (hipStreamSynchronize(xs) != hipSuccess) { err = "copying the depth maps for view spread failed"; return false; }
	return true;
}

// ---- the workers: one estimation thread per device context --------------------------------------------------------------------------------
// Outer iterations over all images (SceneDensify.cpp:3684).  Every device context has a host thread that estimates the context's batches;
// where an outer iteration ends on the main thread (IterPlan::meet) the threads meet, the main thread gathers the maps on the first device,
// filters, hands the filtered maps back and lets the threads go on.
struct Workers {
	Run& r;
	std::mutex mu; std::condition_variable cv;
	std::string error;
	int arrived = 0, released = -1; // workers waiting at the end of an outer iteration; the last iteration the main thread is done with
	std::vector<std::thread> threads;
	explicit Workers(Run& run) : r(run) { for (int d = 0; d < r.nDev; ++d) threads.emplace_back(&Workers::estimate, this, d); }
	~Workers() {
		{ std::lock_guard<std::mutex> g(mu); if (error.empty()) error = "aborted"; }
		cv.notify_all();
		for (auto& t : threads) if (t.joinable()) t.join();
	}
	// main thread: every device has finished the estimates of this outer iteration (or, interleaved mode, is waiting for the main thread to run it)
	bool wait_arrived() {
		std::unique_lock<std::mutex> g(mu);
		cv.wait(g, [&] { return arrived == r.nDev || !error.empty(); });
		if (!error.empty()) { fprintf(stderr, "error: %s\n", error.c_str()); return false; }
		arrived = 0;
		return true;
	}
	void release(int it) { { std::lock_guard<std::mutex> g(mu); released = it; } cv.notify_all(); }
	bool join() {
		for (auto& t : threads) t.join();
		std::lock_guard<std::mutex> g(mu);
		if (!error.empty()) { fprintf(stderr, "error: %s\n", error.c_str()); return false; }
		return true;
	}

private:
	void fail(const std::string& msg) { { std::lock_guard<std::mutex> g(mu); if (error.empty()) error = msg; } cv.notify_all(); }
	bool estimate_batches(int d, const hcmvs_params& pr, const IterPlan& plan) {
		for (size_t b = 0; b < r.batches.size(); ++b) {
			if (r.batches[b].dev != d) continue;
			{ std::lock_guard<std::mutex> g(mu); if (!error.empty()) return false; }
			if (pr.it_external == 0 && !r.loader->wait(b)) { fail("initialisation failed"); return false; }
			std::string err;
			if (!estimate_images(r, d, r.batches[b].ids, pr, err)) { fail(err); return false; }
			if (plan.workerSubmitsFinal) r.saver->submit(r.batches[b].ids); // final maps of this batch: off to the host while the next batch runs
		}
		return true;
	}
	void estimate(int d) {
		if (hipSetDevice(r.devs[(size_t)d].ordinal) != hipSuccess) { fail("hipSetDevice failed in an estimation thread"); return; }
		hcmvs_params pr = r.prm;
		for (int it = 0; it < r.o.estimationItersExternal; ++it) {
			pr.it_external = it;
			const IterPlan plan = plan_iteration(r.o, it, !r.work.empty());
			if (plan.snapshotSpread) { // (one device: this is the only worker, and the previous iteration's filters are done)
				std::string err;
				if (!offer_spread_maps(r, false, err)) { fail(err); return; }
			}
			if (!plan.serial && !estimate_batches(d, pr, plan)) return; // (the interleaved mode runs on the main thread, one device)
			if (plan.meet) { // meet the others; the main thread filters
				std::unique_lock<std::mutex> g(mu);
				++arrived;
				cv.notify_all();
				cv.wait(g, [&] { return released >= it || !error.empty(); });
				if (!error.empty()) return;
			}
		}
	}
};

Run::Run(const Options& opts, double t0) : tStart(t0), o(opts), devs(opts.devices.size()), nDev((int)opts.devices.size()) {
	for (size_t d = 0; d < devs.size(); ++d) devs[d].ordinal = o.devices[d];
}
Run::~Run() {}

// ---- the maps of the whole scene on the first device ----------------------------------------------------------------------------------------
// The first device filters and fuses the whole scene: it holds a copy (g*) of the maps the other devices estimate.  toFirst: owner ->
// first device (gather), else back (scatter, after the post-filters changed them).  Peer copies over xGMI (hipMemcpyPeerAsync); two contexts
// on one GPU (--devices 0,0) copy device to device.  Single process: nothing is replicated, nobody else filters.
bool exchange_maps(Run& r, bool toFirst) {
	hipStream_t xs = r.xs.s;
	const int ord0 = r.devs[0].ordinal;
	if (hipSetDevice(ord0) != hipSuccess) return false; // the copies on the first device are allocated there
	for (uint32_t id : r.todo) {
		ImageData& im = r.images[id];
		const size_t n = im.pixels();
		if (im.dev == 0) { im.gDepth = im.dDepth; im.gNormal = im.dNormal; im.gConf = im.dConf; continue; }
		if (!im.gDepth && (hipMalloc(&im.gDepth, n * 4) != hipSuccess || hipMalloc(&im.gNormal, n * 12) != hipSuccess || hipMalloc(&im.gConf, n * 4) != hipSuccess)) return false;
		const int ord = r.devs[(size_t)im.dev].ordinal;
		float* const dst[3] = {toFirst ? im.gDepth : im.dDepth, toFirst ? im.gNormal : im.dNormal, toFirst ? im.gConf : im.dConf};
		float* const src[3] = {toFirst ? im.dDepth : im.gDepth, toFirst ? im.dNormal : im.gNormal, toFirst ? im.dConf : im.gConf};
		const size_t bytes[3] = {n * 4, n * 12, n * 4};
		for (int k = 0; k < 3; ++k) {
			const hipError_t e = ord == ord0 ? hipMemcpyAsync(dst[k], src[k], bytes[k], hipMemcpyDeviceToDevice, xs)
			                                 : hipMemcpyPeerAsync(dst[k], toFirst ? ord0 : ord, src[k], toFirst ? ord : ord0, bytes[k], xs);
			if (e != hipSuccess) return false;
		}
	}
	return hipStreamSynchronize(xs) == hipSuccess;
}
// the maps and neighbour lists the post-filters, the filter stage and the fusion work on: every image of the scene, on the first device
bool register_maps(Run& r) {
	hcmvs_ctx* ctx = r.ctx;
	for (uint32_t id : r.todo) {
		ImageData& im = r.images[id];
		const std::vector<uint32_t> nb = registered_neighbors(im, r.todo);
		if (hcmvs_set_depthmap_device(ctx, id, im.gDepth ? im.gDepth : im.dDepth, im.gNormal ? im.gNormal : im.dNormal, im.gConf ? im.gConf : im.dConf, im.dMin, im.dMax) != HCMVS_OK ||
		    hcmvs_set_neighbors(ctx, id, nb.data(), (int32_t)nb.size()) != HCMVS_OK) {
			fprintf(stderr, "error: registering the maps of image %u failed (%s)\n", id, hcmvs_last_error(ctx));
			return false;
		}
	}
	return true;
}
// gather the maps on the first device, register them, do `body` there and -- where it changed the maps -- hand them back to their devices
template <typename Body>
bool on_first_device(Run& r, bool handBack, Body body) {
	if (!exchange_maps(r, true)) { fprintf(stderr, "error: gathering the depth maps on device %d failed\n", r.devs[0].ordinal); return false; }
	if (!register_maps(r)) return false;
	if (!body()) return false;
	if (handBack && !exchange_maps(r, false)) { fprintf(stderr, "error: handing the filtered depth maps back to their devices failed\n"); return false; }
	return true;
}
void release_all(Run& r) {
	for (auto& im : r.images) {
		(void)hipSetDevice(r.devs[(size_t)im.dev].ordinal);
		for (float* q : {im.dDepth, im.dNormal, im.dConf, im.dHintDepth, im.dHintNormal}) if (q) (void)hipFree(q);
		if (im.dev != 0) { (void)hipSetDevice(r.devs[0].ordinal); for (float* q : {im.gDepth, im.gNormal, im.gConf}) if (q) (void)hipFree(q); }
	}
	for (auto& d : r.devs) hcmvs_destroy(d.ctx);
}

// ---- the phases of a run, in the order main() calls them ------------------------------------------------------------------------------------
// The device contexts come up (HIP runtime start, ~0.4 s) while the scene is read and the views are selected on the host.
void start_contexts(Run& r) {
	r.creator.t = std::thread([&r] { for (auto& d : r.devs) d.createRc = hcmvs_create(d.ordinal, &d.ctx); });
}
// The scene file and the headers of the images: the working size and the camera of every image are known before a pixel is decoded, which
// is all the view selection needs
bool read_scene(Run& r) {
	const Options& o = r.o;
	if (!load_mvs(o.input, r.platforms, r.mimages, r.verts)) { fprintf(stderr, "error: can not load '%s'\n", o.input.c_str()); return false; }
	r.images.resize(r.mimages.size());
	r.paths.resize(r.mimages.size());
	for (size_t i = 0; i < r.mimages.size(); ++i) {
		ImageData& im = r.images[i];
		const MvsImage& mi = r.mimages[i];
		im.name = mi.name; im.id = (uint32_t)i;
		if (mi.poseID == 0xFFFFFFFFu || mi.platformID >= r.platforms.size()) continue; // uncalibrated
		const MvsPlatform& p = r.platforms[mi.platformID];
		const MvsCamera& c = p.cams[mi.cameraID];
		const MvsPose& q = p.poses[mi.poseID];
		r.paths[i] = im.name[0] == '/' ? im.name : dirname_of(o.input) + "/" + im.name;
		int fw = 0, fh = 0;
		if (!pnm_size(r.paths[i], fw, fh)) { fprintf(stderr, "error: failed loading image '%s' (binary PPM/PGM expected)\n", r.paths[i].c_str()); return false; }
		// SceneDensify.cpp:3612-3615: one INTER_AREA resize to the resolution level's size, within [min-resolution, max-resolution]
		working_size(fw, fh, (unsigned)std::max(0, o.resolutionLevel), (unsigned)std::max(1, o.minResolution), (unsigned)std::max(1, o.maxResolution), im.w, im.h);
		image_camera(c, q, im.w, im.h, im.cam); // K rescaled to the working resolution
		im.valid = true;
		++r.nValid;
	}
	return true;
}
// The view selection of every image, all cores (every image writes only its own lists; the selection reads cameras and sizes, no pixels;
// SceneDensify.cpp:3590-3634 is an OpenMP loop too)
void select_all_views(Run& r) {
	r.selected.assign(r.images.size(), 0);
#pragma omp parallel for schedule(dynamic, 1)
	for (long i = 0; i < (long)r.images.size(); ++i)
		if (r.images[(size_t)i].valid) r.selected[(size_t)i] = select_views(r.images, r.verts, (uint32_t)i, 12, r.o.numberViews) ? 1 : 0;
}
bool contexts_ready(Run& r) {
	const Options& o = r.o;
	r.creator.t.join();
	for (auto& d : r.devs)
		if (d.createRc != HCMVS_OK) { fprintf(stderr, "error: device %d is not a usable MI355X (there is no CPU path)\n", d.ordinal); return false; }
	r.ctx = r.devs[0].ctx;
	if (hipSetDevice(o.device) != hipSuccess) { fprintf(stderr, "error: hipSetDevice failed\n"); return false; }
	if (r.nDev > 1 && o.geoConsistency) { fprintf(stderr, "error: --geo-consistency 1 runs on one device: every estimate reads the depth maps of its source views, which other devices would hold (drop --devices)\n"); return false; }
	if (r.nDev > 1 && o.viewspread) { fprintf(stderr, "error: --n-viewspread 1 runs on one device: every estimate reads the depth maps of its source views, which other devices would hold (drop --devices)\n"); return false; }
	if (r.nDev > 1 && o.postFilterInterleave) { fprintf(stderr, "error: --n-postfilter-interleave 1 estimates one image at a time and runs on one device (drop --devices)\n"); return false; }
	return true;
}
// the images that get maps, and the parameters of their estimates
void list_todo(Run& r) {
	const Options& o = r.o;
	for (auto& im : r.images) {
		if (!im.valid) continue;
		if (!r.selected[im.id]) {
			if (o.verbosity > 1) printf("Reference image %3u has not enough images in view\n", im.id);
			continue;
		}
		r.todo.push_back(im.id);
		if (o.verbosity > 2) { // SceneDensify.cpp:376-384
			printf("Reference image %3u paired with %zu views:", im.id, im.srcs.size());
			for (uint32_t s : im.srcs) {
				float scl = 1.f;
				for (const auto& nb : im.neighbors) if (nb.id == s) scl = nb.scale;
				printf(" %3u(%.2fscl)", s, scl);
			}
			printf(" (%zu shared points)\n", im.points.size());
		}
	}
	hcmvs_default_params(&r.prm);
	r.prm.adapthalfwin = o.adaptHalfWin; r.prm.n_estimation_iters = o.estimationIters; r.prm.n_external_iters = o.estimationItersExternal;
	r.prm.propagate_halfwin = o.propagateHalfWin; r.prm.propagate_step = o.propagateStep; r.prm.photometric_flow = o.photometricFlow; r.prm.seed = o.seed;
}
// Deal the images to the devices and see that every device's share fits (plan_deal, plan_device_budget): the batch shrinks until every
// device fits; a scene that does not fit at one image per launch is refused here, before anything is uploaded
bool deal_and_budget(Run& r) {
	Options& o = r.o;
	r.deal = plan_deal(r.images, r.todo, r.nDev);
	for (uint32_t id : r.todo) r.images[id].dev = r.deal.dev[id];
	for (int d = 0; d < r.nDev; ++d) {
		const int ordinal = r.devs[(size_t)d].ordinal;
		size_t freeB = 0, totalB = 0;
		HIPOK(hipSetDevice(ordinal));
		HIPOK(hipMemGetInfo(&freeB, &totalB));
		const DeviceBudget b = plan_device_budget(r.images, r.todo, r.deal, d, freeB, o);
		if (!b.fits) {
			fprintf(stderr, "error: the scene does not fit device %d: %.1f GiB needed for its share (%zu of %zu images; maps, images, source footprints%s), "
			                "%.1f GiB free.  Use more devices (--devices), a coarser --resolution-level or fewer --number-views\n",
			        ordinal, b.needed() / 1073741824.0, b.ownImages, r.todo.size(), d == 0 ? ", the whole scene's maps, fusion tables and cloud" : "", freeB / 1073741824.0);
			return false;
		}
		o.batch = std::min(o.batch, b.batch);
		if (o.verbosity > 2) printf("Device %d (context %d of %d): %.1f GiB resident + %.1f GiB per batch of %d, %.1f GiB free\n", ordinal, d, r.nDev,
		                            b.resident / 1073741824.0, (size_t)b.batch * b.perImage / 1073741824.0, b.batch, freeB / 1073741824.0);
	}
	HIPOK(hipSetDevice(o.device));
	return true;
}
// skip-if-exists resume (SceneDensify.cpp:3865-3880: "try to load already compute depth-map for this image"): an image whose
// final depth map of this size is in the working folder is loaded instead of estimated
bool resume_finished(Run& r) {
	const Options& o = r.o;
	std::vector<char> resumed(r.images.size(), 0);
	for (uint32_t id : r.todo) {
		DmapFile hdr;
		if (o.resume && load_dmap(map_path(o.workdir, "/depth%04u.dmap", id), hdr, 7, true) && hdr.w == r.images[id].w && hdr.h == r.images[id].h) resumed[id] = 1;
		else { r.work.push_back(id); r.devs[(size_t)r.images[id].dev].work.push_back(id); }
	}
	for (uint32_t id : r.todo) {
		if (!resumed[id]) continue;
		ImageData& im = r.images[id];
		const std::string path = map_path(o.workdir, "/depth%04u.dmap", id);
		DmapFile m;
		if (!load_dmap(path, m, 7)) { fprintf(stderr, "error: invalid depth-map '%s'\n", path.c_str()); return false; }
		const size_t n = im.pixels();
		im.dMin = m.dMin; im.dMax = m.dMax;
		HIPOK(hipSetDevice(r.devs[(size_t)im.dev].ordinal));
		HIPOK(hipMalloc(&im.dDepth, n * 4)); HIPOK(hipMalloc(&im.dNormal, n * 12)); HIPOK(hipMalloc(&im.dConf, n * 4));
		HIPOK(hipMemcpy(im.dDepth, m.d.data(), n * 4, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(im.dNormal, m.n.data(), n * 12, hipMemcpyHostToDevice));
		HIPOK(hipMemcpy(im.dConf, m.c.data(), n * 4, hipMemcpyHostToDevice));
		if (o.verbosity > 1) printf("Depth-map for image %3u loaded from '%s' (not estimated again)\n", id, path.c_str());
	}
	HIPOK(hipSetDevice(o.device));
	return true;
}
void plan_image_batches(Run& r) {
	std::vector<std::vector<uint32_t>> work;
	for (const auto& d : r.devs) work.push_back(d.work);
	r.batches = plan_batches(r.images, work, r.o.batch);
}
// decode + resize + gray conversion of one image, and its upload to every device that needs it
void decode_and_upload(Run& r, size_t t) {
	ImageData& im = r.images[t];
	int fw = 0, fh = 0;
	std::vector<uint8_t> bgr;
	if (!load_pnm(r.paths[t], fw, fh, bgr)) { std::lock_guard<std::mutex> g(r.errMu); r.loadError = "failed loading image '" + r.paths[t] + "'"; return; }
	if (fw != im.w || fh != im.h) resize_area_bgr(fw, fh, bgr, im.w, im.h);
	// gray and colour image go into page-locked memory of this thread: what is left for the (serial) upload is the transfer
	static thread_local struct Pinned { char* p = nullptr; size_t cap = 0; } pin; // lives as long as its thread; the process ends with them
	const size_t px = im.pixels(), need = px * 4 + px * 3;
	if (pin.cap < need) {
		if (pin.p) (void)hipHostFree(pin.p);
		pin.p = nullptr; pin.cap = 0;
		if (hipSetDevice(r.o.device) == hipSuccess && hipHostMalloc((void**)&pin.p, need, hipHostMallocPortable) == hipSuccess) pin.cap = need;
		else { (void)hipGetLastError(); pin.p = nullptr; }
	}
	std::vector<float> grayVec;
	float* gray = (float*)pin.p;
	uint8_t* bgrUp = pin.p ? (uint8_t*)(pin.p + px * 4) : bgr.data();
	if (!pin.p) { grayVec.resize(px); gray = grayVec.data(); } // no page-locked memory to be had: the library stages the copy
	else memcpy(bgrUp, bgr.data(), px * 3);
	for (size_t k = 0; k < px; ++k) // Types.inl:2354-2400 toGray, normalised
		gray[k] = (0.114f * bgr[3 * k] + 0.587f * bgr[3 * k + 1] + 0.299f * bgr[3 * k + 2]) / 255.f;
	for (size_t d = 0; d < r.devs.size(); ++d) {
		// a device gets the gray image of its own reference images and of their source views; the first device also gets camera + colour image
		// of every other image (a fuse-only view: hcmvs_upload_view with gray = NULL), because it filters and fuses the whole scene
		const bool g = r.deal.needGray[d][t] != 0;
		if (!g && d != 0) continue; // this device never touches the image
		std::lock_guard<std::mutex> lk(r.devs[d].upMu); // one HIP stream per context: uploads one after the other, while the other cores decode
		if (hcmvs_upload_view(r.devs[d].ctx, im.id, im.w, im.h, g ? gray : nullptr, bgrUp, im.cam.K, im.cam.R, im.cam.C) != HCMVS_OK) {
			std::lock_guard<std::mutex> e(r.errMu);
			if (r.loadError.empty()) r.loadError = std::string("upload of image '") + r.paths[t] + "' failed: " + hcmvs_last_error(r.devs[d].ctx);
		}
	}
}
// The loader starts on the first batches' initial maps (the triangulated ones need cameras and sparse points only), then the images are
// decoded on all cores; an image goes to the device as soon as it is decoded
bool load_images(Run& r) {
	const Options& o = r.o;
	r.loader.reset(new Loader(r));
	const double tDecode = now_s();
	const long N = (long)r.images.size();
#pragma omp parallel for schedule(dynamic, 1)
	for (long t = 0; t < N; ++t)
		if (r.images[(size_t)t].valid) decode_and_upload(r, (size_t)t);
	if (o.verbosity > 2) printf("Start-up: %.2f s until the images are decoded (scene file, headers, view selection, device context), %.2f s decoding + uploading them\n", tDecode - r.tStart, now_s() - tDecode);
	if (!r.loadError.empty()) { fprintf(stderr, "error: %s\n", r.loadError.c_str()); return false; }
	if (o.verbosity > 1) printf("Scene loaded: %zu images (%u calibrated), %zu sparse points\n", r.images.size(), r.nValid, r.verts.size());
	r.tLoaded = now_s();
	return true;
}
// neighbours whose footprint scale differs by >= 15 % are resampled on the device and registered as views of their own
// (DepthData::ViewData::ScaleImage + Image::GetCamera, SceneDensify.cpp:372-374); one copy per (image, new size) and device
bool rescale_neighbours(Run& r) {
	std::map<std::pair<uint32_t, std::pair<int, int>>, uint32_t> scaled;
	std::vector<std::map<uint32_t, bool>> made((size_t)r.nDev);
	uint32_t nextId = 0x8000;
	for (uint32_t id : r.todo) {
		ImageData& im = r.images[id];
		im.srcImages = im.srcs;
		for (size_t k = 0; k < im.srcs.size(); ++k) {
			if (im.srcScale[k] == 1.f) continue;
			const ImageData& sv = r.images[im.srcs[k]];
			const std::pair<int, int> size((int)std::lrint((double)sv.w * im.srcScale[k]), (int)std::lrint((double)sv.h * im.srcScale[k]));
			const auto key = std::make_pair(sv.id, size);
			auto it = scaled.find(key);
			if (it == scaled.end()) {
				if (nextId >= 65536) { fprintf(stderr, "error: too many resampled neighbour views\n"); return false; }
				it = scaled.emplace(key, nextId++).first;
			}
			if (!made[(size_t)im.dev].count(it->second)) {
				hcmvs_ctx* dctx = r.devs[(size_t)im.dev].ctx;
				if (hcmvs_rescale_view(dctx, sv.id, it->second, im.srcScale[k]) != HCMVS_OK) { fprintf(stderr, "error: resampling image %u failed (%s)\n", sv.id, hcmvs_last_error(dctx)); return false; }
				if (r.o.verbosity > 2) printf("Image %3u resampled by %.2f to %dx%d as view %u\n", sv.id, im.srcScale[k], size.first, size.second, it->second);
				made[(size_t)im.dev][it->second] = true;
			}
			im.srcs[k] = it->second;
		}
	}
	HIPOK(hipSetDevice(r.o.device));
	return true;
}
// --ignore-mask-label (DepthEstimator::ImportIgnoreMask, DepthMap.cpp:319-348): the labels split at every ',' (empty tokens kept,
// Util::strSplit) and read with atoi; every image to estimate gets the keep-mask of its label image on the context that estimates it
bool set_ignore_masks(Run& r) {
	const Options& o = r.o;
	if (o.ignoreMaskLabel.empty()) return true;
	std::vector<int32_t> labels;
	for (size_t b = 0;;) {
		const size_t e = o.ignoreMaskLabel.find(',', b);
		labels.push_back((int32_t)atoi(o.ignoreMaskLabel.substr(b, e == std::string::npos ? std::string::npos : e - b).c_str()));
		if (e == std::string::npos) break;
		b = e + 1;
	}
	size_t nMasked = 0, pxAll = 0, pxIgnored = 0;
	for (uint32_t id : r.todo) {
		const ImageData& im = r.images[id];
		// the fork's rule (Scene.cpp:119-126): getFilePath(name) + "/seman/" + getFileName(name) + ".quad.png", read here as its binary
		// Netpbm siblings.  A name without a folder resolves against the image's own folder (the fork makes it root-absolute).
		const size_t sl = im.name.find_last_of('/');
		std::string stem = sl == std::string::npos ? im.name : im.name.substr(sl + 1);
		if (stem.find_last_of('.') != std::string::npos) stem = stem.substr(0, stem.find_last_of('.'));
		const std::string base = dirname_of(r.paths[id]) + "/seman/" + stem + ".quad";
		std::vector<uint16_t> lab;
		int lw = 0, lh = 0;
		std::string used;
		for (const char* ext : {".pgm", ".ppm"})
			if (load_labels(base + ext, lw, lh, lab)) { used = base + ext; break; }
		if (used.empty()) {
			if (o.verbosity > 1) fprintf(stderr, "warning: can not load the segmentation mask '%s.png' (tried '%s.pgm' and '%s.ppm'): image %u is not masked\n",
			                             base.c_str(), base.c_str(), base.c_str(), id);
			continue;
		}
		hcmvs_ctx* dctx = r.devs[(size_t)im.dev].ctx;
		std::vector<uint8_t> keep(im.pixels());
		if (hcmvs_set_ignore_mask(dctx, id, lab.data(), lw, lh, labels.data(), (int32_t)labels.size()) != HCMVS_OK ||
		    hcmvs_get_ignore_mask(dctx, id, keep.data()) != HCMVS_OK) {
			fprintf(stderr, "error: the ignore mask of image %u failed (%s)\n", id, hcmvs_last_error(dctx));
			return false;
		}
		++nMasked; pxAll += keep.size();
		pxIgnored += (size_t)std::count(keep.begin(), keep.end(), (uint8_t)0);
	}
	HIPOK(hipSetDevice(o.device));
	if (o.verbosity > 1)
		printf("Ignore mask (labels %s): %zu of %zu images masked, %.2f %% of their pixels ignored\n", o.ignoreMaskLabel.c_str(), nMasked, r.todo.size(),
		       pxAll ? 100.0 * (double)pxIgnored / (double)pxAll : 0.0);
	return true;
}
// --plane-priors 1: the label image of every image to estimate, found as the ignore mask's is (seman/<stem>.quad.pgm|ppm), registers the
// region of the label 255 on the context that estimates the image; an image without a label file has no prior
bool set_prior_regions(Run& r) {
	const Options& o = r.o;
	if (!o.planePriors) return true;
	if (priors_never_used(o) && o.verbosity > 1)
		fprintf(stderr, "note: --plane-priors 1 needs two outer iterations or more (--n-EstimationIters-external %d): no prior is generated\n", o.estimationItersExternal);
	if (!o.exportPriors.empty()) (void)mkdir(o.exportPriors.c_str(), 0777);
	hcmvs_prior_params pp;
	pp.para_prior = o.paraPrior; pp.sigma_prior = o.sigmaPrior; pp.photo2geo = o.photo2geo;
	for (DeviceCtx& d : r.devs)
		if (hcmvs_set_prior_params(d.ctx, &pp) != HCMVS_OK) { fprintf(stderr, "error: %s\n", hcmvs_last_error(d.ctx)); return false; }
	size_t nRegions = 0;
	for (uint32_t id : r.work) {
		ImageData& im = r.images[id];
		const size_t sl = im.name.find_last_of('/');
		std::string stem = sl == std::string::npos ? im.name : im.name.substr(sl + 1);
		if (stem.find_last_of('.') != std::string::npos) stem = stem.substr(0, stem.find_last_of('.'));
		const std::string base = dirname_of(r.paths[id]) + "/seman/" + stem + ".quad";
		std::vector<uint16_t> lab;
		int lw = 0, lh = 0;
		bool found = false;
		for (const char* ext : {".pgm", ".ppm"})
			if (load_labels(base + ext, lw, lh, lab)) { found = true; break; }
		if (!found) {
			if (o.verbosity > 1) fprintf(stderr, "warning: no label image '%s.pgm' or '%s.ppm': image %u gets no plane prior\n", base.c_str(), base.c_str(), id);
			continue;
		}
		hcmvs_ctx* dctx = r.devs[(size_t)im.dev].ctx;
		if (hcmvs_set_prior_region(dctx, id, lab.data(), lw, lh, 255) != HCMVS_OK) { fprintf(stderr, "error: the prior region of image %u failed (%s)\n", id, hcmvs_last_error(dctx)); return false; }
		im.hasRegion = true;
		++nRegions;
	}
	HIPOK(hipSetDevice(o.device));
	if (o.verbosity > 1)
		printf("Plane priors: %zu of %zu images to estimate have a label image; probability %g, epsilon %g, min-points %g, seed %llu\n", nRegions, r.work.size(),
		       (double)o.ransacProbability, (double)o.ransacEpsilon, (double)o.ransacMinPoints, o.sampleSeed);
	if (o.verbosity > 1 && o.planeClusters) printf("Plane clusters: a plane keeps the largest connected component of its inliers, cells of %g average spacings\n", (double)o.ransacCluster);
	if (o.verbosity > 1 && o.planeRefit) printf("Plane refit: the winning plane of a round is refitted by %d least-squares steps over its inliers in a quarter of the band\n", o.planeRefit);
	return true;
}
// --depth-priors <folder>: <folder>/depth%04u.prior.dmap per image that is estimated, a raw 'DR' depth map of the image's size at the run's
// resolution level; only the depth is read.  A file of another size is an error naming it; an image without a file has no prior.
bool load_depth_priors(Run& r) {
	const Options& o = r.o;
	if (o.depthPriors.empty()) return true;
	if (priors_never_used(o) && o.verbosity > 1)
		fprintf(stderr, "note: --depth-priors needs two outer iterations or more (--n-EstimationIters-external %d): the priors are never used\n", o.estimationItersExternal);
	hcmvs_prior_params pp;
	pp.para_prior = o.paraPrior; pp.sigma_prior = o.sigmaPrior; pp.photo2geo = o.photo2geo;
	for (DeviceCtx& d : r.devs)
		if (hcmvs_set_prior_params(d.ctx, &pp) != HCMVS_OK) { fprintf(stderr, "error: %s\n", hcmvs_last_error(d.ctx)); return false; }
	size_t nPriors = 0;
	for (uint32_t id : r.work) {
		ImageData& im = r.images[id];
		const std::string path = prior_path(o, id);
		sceneio::DmapFile m;
		if (!sceneio::load_dmap(path, m, 1, true)) continue; // no file (or not a depth map): no prior
		if (m.w != im.w || m.h != im.h) {
			fprintf(stderr, "error: the depth prior '%s' is %dx%d, image %u is %dx%d at this resolution level\n", path.c_str(), m.w, m.h, id, im.w, im.h);
			return false;
		}
		if (!sceneio::load_dmap(path, m, 1)) { fprintf(stderr, "error: invalid depth prior '%s'\n", path.c_str()); return false; }
		im.prior.swap(m.d);
		++nPriors;
	}
	if (o.verbosity > 1)
		printf("Depth priors (%s): %zu of %zu images to estimate have one; para_prior %g, sigma_prior %g, photo2geo %d\n", o.depthPriors.c_str(), nPriors, r.work.size(),
		       (double)o.paraPrior, (double)o.sigmaPrior, o.photo2geo);
	return true;
}
bool start_saver_and_workers(Run& r) {
	hcmvs_ctx* ctx = r.ctx;
	(void)mkdir((r.o.workdir + "/depthmap").c_str(), 0777);
	(void)mkdir((r.o.workdir + "/normalmap").c_str(), 0777);
	r.saver.reset(new Saver(r));
	r.tInit = now_s();
	HIPOK(hipStreamCreateWithFlags(&r.xs.s, hipStreamNonBlocking));
	if (r.o.viewspread) CHK(hcmvs_set_viewspread(ctx, 1));
	if (r.o.geoConsistency) { // the geometric-consistency term: the source views' maps are offered as for view spread (plan_iteration)
		const hcmvs_geo_params gp = geo_params(r.o);
		CHK(hcmvs_set_geo_params(ctx, &gp));
		printf("Geometric consistency: para_tapa %g (texture < %g), para_tapa2 %g (texture < %g), photo2geo %d, max_px %g\n", (double)gp.para_tapa,
		       (double)gp.txthreshold, (double)gp.para_tapa2, (double)gp.txthreshold2, gp.photo2geo, (double)gp.max_px);
	}
	r.workers.reset(new Workers(r));
	return true;
}
int min_views_fuse(const Run& r) { return std::min<int>(r.o.numberViewsFuse, (int)r.images.size()); }
// The interleaved schedule, on the first device with every map registered: the reference's order, exactly (single-thread event loop,
// SceneDensify.cpp:3889-3965: EVTEstimateDepthMap(k) queues EVTOptimizeDepthMap(k) FIRST): image k is filtered right after its own
// estimate, so its fusion sees the images > k as the previous outer iteration left them and zeroes depths in them before they are
// estimated again.  One image per launch: the exact mode, not the fast one
bool estimate_image_after_image(Run& r, int it, const IterPlan& plan, double tp) {
	hcmvs_ctx* ctx = r.ctx;
	const Options& o = r.o;
	if (plan.liveSpread) {
		std::string err;
		if (!offer_spread_maps(r, true, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return false; }
	}
	hcmvs_params pr = r.prm;
	pr.it_external = it;
	uint64_t filledAll = 0;
	double tf = 0;
	for (uint32_t id : r.work) {
		std::string err;
		if (!estimate_images(r, 0, std::vector<uint32_t>(1, id), pr, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return false; }
		if (!plan.filtered) continue; // (view spread alone: image after image, nothing to filter in this outer iteration)
		const double t0 = now_s();
		uint64_t filled = 0;
		CHK(hcmvs_postfilter(ctx, id, r.deal.fuseOrder.data(), (int32_t)r.deal.fuseOrder.size(), min_views_fuse(r), 0.01f, 25.f, 7, &filled));
		filledAll += filled;
		tf += now_s() - t0;
	}
	r.tPostfilter += tf;
	if (o.verbosity > 1 && !plan.filtered) printf("Depth-maps estimated image after image in outer iteration %d (the reference's order, view spread on the live maps) (%.2f s)\n", it, now_s() - tp);
	else if (o.verbosity > 1) printf("Depth-maps estimated and filtered image after image in outer iteration %d (the reference's order): %llu pixels filled "
	                            "(%.2f s, %.2f s of it post-filters)\n", it, (unsigned long long)filledAll, now_s() - tp, tf);
	return true;
}
// the batch schedule of the post-filters: every image of the outer iteration has been estimated, now
// they are filtered one image after the other (hcmvs_postfilter_sequence keeps the whole chain on the device)
bool postfilter_all(Run& r, int it, double tp) {
	hcmvs_ctx* ctx = r.ctx;
	uint64_t filledAll = 0;
	CHK(hcmvs_postfilter_sequence(ctx, r.work.data(), (int32_t)r.work.size(), r.deal.fuseOrder.data(), (int32_t)r.deal.fuseOrder.size(), min_views_fuse(r), 0.01f, 25.f, 7, &filledAll));
	r.tPostfilter += now_s() - tp;
	if (r.o.verbosity > 1) printf("Depth-maps filtered after outer iteration %d: fuse-consistency mask + gap interpolation, %llu pixels filled (%.2f s)\n", it,
	                              (unsigned long long)filledAll, now_s() - tp);
	return true;
}
// The main thread's part of the outer iterations (plan_iteration says which of them have one): SceneDensify.cpp:3916, 3939-3958 -- with
// --n-nOptimize's REMOVE_SPECKLES | FILL_GAPS bits, after the estimates of outer iterations 1 and 2 every image goes through
// RemoveSmallSegments (in the fork: a whole fusion pass over the current maps of all images) and GapInterpolation
bool run_outer_iterations(Run& r) {
	for (int it = 0; it < r.o.estimationItersExternal; ++it) {
		const IterPlan plan = plan_iteration(r.o, it, !r.work.empty());
		if (!plan.meet) continue;
		if (!r.workers->wait_arrived()) return false;
		const double tp = now_s();
		if (!on_first_device(r, true, [&] { return plan.serial ? estimate_image_after_image(r, it, plan, tp) : postfilter_all(r, it, tp); })) return false;
		if (plan.mainSubmitsFinal) r.saver->submit(r.work); // (--n-filter: the files are written after the filter stage)
		r.workers->release(it);
	}
	return true;
}
bool finish_estimates(Run& r) {
	const Options& o = r.o;
	if (!r.workers->join()) return false;
	r.loader->join();
	double pixels = 0;
	for (uint32_t id : r.work) pixels += (double)r.images[id].pixels();
	for (auto& d : r.devs) if (hcmvs_synchronize(d.ctx) != HCMVS_OK) { fprintf(stderr, "error: %s\n", hcmvs_last_error(d.ctx)); return false; }
	r.tEstimated = now_s();
	if (o.verbosity > 1)
		printf("Depth-maps estimated: %zu images (%zu resumed), %d outer x %d inner sweeps in %.2f s (%.2f Mpix/s per outer iteration; post-filters %.2f s of it); "
		       "loading + view selection %.2f s, set-up %.2f s\n",
		       r.work.size(), r.todo.size() - r.work.size(), o.estimationItersExternal, o.estimationIters, r.tEstimated - r.tInit,
		       pixels * o.estimationItersExternal / std::max(1e-9, r.tEstimated - r.tInit - r.tPostfilter) / 1e6, r.tPostfilter, r.tLoaded - r.tStart, r.tInit - r.tLoaded);
	if (o.verbosity > 1 && o.speckleSize > 0)
		printf("Speckle filter (segments below %d pixels, depth difference below %g): %llu segments, %llu small, %llu of %llu pixels removed, %.3f ms on the device\n",
		       o.speckleSize, (double)o.speckleDiff, (unsigned long long)r.speckle.n_segments, (unsigned long long)r.speckle.n_small,
		       (unsigned long long)r.speckle.n_removed, (unsigned long long)r.speckle.n_valid, r.speckle.ms_device);
	return true;
}
// --n-filter: the filter stage (Scene::DenseReconstructionFilter, SceneDensify.cpp:4100-4185 -- the block the fork switched off at :3721-3756):
// every image that has maps, the ones loaded through skip-if-exists included, against the first 8 of its neighbours that have maps
// (:4116-4131), all from the maps as the estimates left them; then the filtered maps are saved (:4173) and the fusion works on them.
// On the first device, after the gather that also precedes the fusion.
bool filter_stage(Run& r) {
	const Options& o = r.o;
	if (!stage_submits_final(o) || r.todo.empty()) return true;
	hcmvs_ctx* ctx = r.ctx;
	const double tf = now_s();
	// nMinViewsFilter 2, nMinViewsFilterAdjust 1, clamped to the calibrated images - 1 (SceneDensify.cpp:3014-3015)
	const int nMinViewsFilter = std::min<int>(2, (int)r.nValid - 1), nMinViewsFilterAdjust = std::min<int>(1, (int)r.nValid - 1);
	hcmvs_filter_stats fs;
	memset(&fs, 0, sizeof fs);
	if (!on_first_device(r, true, [&] { CHK(hcmvs_filter_sequence(ctx, r.todo.data(), (int32_t)r.todo.size(), 8, o.nFilter == 1 ? 1 : 0, nMinViewsFilter, nMinViewsFilterAdjust, 0.01f, &fs)); return true; })) return false;
	r.saver->submit(r.todo);
	if (o.verbosity > 1)
		printf("Depth-maps filtered: %u images, %llu/%llu depths discarded (%u skipped) in %.2f s (%s; %.2f ms on the device, batches of up to %u images)\n", fs.n_filtered,
		       (unsigned long long)fs.n_discarded, (unsigned long long)fs.n_processed, fs.n_skipped, now_s() - tf, o.nFilter == 1 ? "adjust" : "strict", fs.ms_device, fs.batch);
	return true;
}
// the fusion mutates the depth maps: every final map must be on the host first (the files may still be on their way)
bool final_maps_on_host(Run& r) {
	r.saver->close();
	if (!r.saver->wait_copied()) return false;
	r.tCopied = now_s();
	return true;
}
// --fusion-mode 1, or nothing to fuse: the depth maps are the result
bool finish_without_fusion(Run& r) {
	if (!r.saver->wait_written()) return false;
	if (r.o.verbosity > 1) printf("Depth-maps saved (%.2f s after the last estimate)\n", now_s() - r.tEstimated);
	release_all(r);
	return true;
}

// the complete PointCloud: points, view lists + weights (PointCloud::pointViews / pointWeights), colours, normals
struct Cloud {
	RawArray<float> xyz, nrm; RawArray<uint8_t> bgr; RawArray<uint32_t> nviews;
	RawArray<uint32_t> viewIds; RawArray<float> viewWeights;
	uint64_t nPoints = 0, nDepths = 0;
	explicit Cloud(const CloudSize& s) : xyz(s.capacity * 3), nrm(s.capacity * 3), bgr(s.capacity * 3), nviews(s.capacity), viewIds(s.viewCapacity), viewWeights(s.viewCapacity) {}
	bool allocated() { return xyz.data() && nrm.data() && bgr.data() && nviews.data() && viewIds.data() && viewWeights.data(); }
};
// the counting pass of a large scene (fusion_counts_first): `size` becomes what the cloud needs, exactly
bool count_cloud(Run& r, CloudSize& size, uint64_t& countedDepths) {
	hcmvs_ctx* ctx = r.ctx;
	const Options& o = r.o;
	hcmvs_cloud cnt;
	memset(&cnt, 0, sizeof cnt);
	CHK(hcmvs_set_fuse_order(ctx, o.fuseOrder));
	CHK(hcmvs_fuse_cloud(ctx, r.deal.fuseOrder.data(), (int32_t)r.deal.fuseOrder.size(), min_views_fuse(r), 0.01f, 25.f, o.depthweight, o.normalweight, &cnt));
	if (o.verbosity > 2) printf("Fusion counted first: %llu points, %llu view entries (worst case reserved otherwise: %llu / %llu)\n", (unsigned long long)cnt.n_points,
	                            (unsigned long long)cnt.n_view_entries, (unsigned long long)size.capacity, (unsigned long long)size.viewCapacity);
	size.capacity = cnt.n_points + 1; size.viewCapacity = cnt.n_view_entries + 1;
	countedDepths = cnt.n_depths; // the depths the fusion visited before it invalidated any (SceneDensify.cpp:3461 logs that number)
	return true;
}
// fuse: best connected images first (SceneDensify.cpp:3285-3302)
bool fuse_cloud(Run& r, Cloud& c, const CloudSize& size, uint64_t countedDepths) {
	hcmvs_ctx* ctx = r.ctx;
	const Options& o = r.o;
	CHK(hcmvs_set_fuse_order(ctx, o.fuseOrder));
	hcmvs_cloud cl;
	memset(&cl, 0, sizeof cl);
	cl.capacity = size.capacity; cl.xyz = c.xyz.data(); cl.normal = c.nrm.data(); cl.bgr = c.bgr.data(); cl.n_views = c.nviews.data();
	cl.views_capacity = size.viewCapacity; cl.view_ids = c.viewIds.data(); cl.view_weights = c.viewWeights.data();
	CHK(hcmvs_fuse_cloud(ctx, r.deal.fuseOrder.data(), (int32_t)r.deal.fuseOrder.size(), min_views_fuse(r), 0.01f, 25.f, o.depthweight, o.normalweight, &cl));
	c.nPoints = cl.n_points; c.nDepths = countedDepths ? countedDepths : cl.n_depths;
	c.xyz.shrink(c.nPoints * 3); c.nrm.shrink(c.nPoints * 3); c.bgr.shrink(c.nPoints * 3); c.nviews.shrink(c.nPoints);
	c.viewIds.shrink(cl.n_view_entries); c.viewWeights.shrink(cl.n_view_entries);
	// --estimate-colors / --estimate-normals: 2 = estimated during fusion (above), 1 = re-estimated on the final cloud
	// (SceneDensify.cpp:3544, 3567-3572), 0 = none
	if (o.estimateColors == 1) CHK(hcmvs_estimate_point_colors(ctx, c.nPoints, c.xyz.data(), c.nviews.data(), c.viewIds.data(), c.bgr.data()));
	if (o.estimateNormals == 1) CHK(hcmvs_estimate_point_normals(ctx, c.nPoints, c.xyz.data(), c.nviews.data(), c.viewIds.data(), 16, c.nrm.data()));
	if (o.estimateColors == 0) c.bgr.clear();
	if (o.estimateNormals == 0) c.nrm.clear();
	return true;
}
// the scene and the point cloud, side by side
bool save_cloud(Run& r, const Cloud& c) {
	const Options& o = r.o;
	const std::string base = o.output.substr(0, o.output.rfind('.'));
	bool okMvs = false, okPly = false;
	{
		std::thread tm([&] { okMvs = save_mvs(o.output, r.platforms, r.mimages, c.xyz, c.nrm, c.bgr, c.nviews, c.viewIds, c.viewWeights); });
		okPly = save_ply(base + ".ply", c.xyz, c.nrm, c.bgr);
		tm.join();
	}
	if (!okMvs || !okPly) { fprintf(stderr, "error: can not write the output files\n"); return false; }
	return true;
}
// The fusion, with the maps of every image on the first device (the exchange before fusion); then the outputs
bool fuse_and_save(Run& r) {
	const Options& o = r.o;
	CloudSize size = cloud_worst_case(r.images, r.todo, o.numberViewsFuse);
	uint64_t countedDepths = 0;
	if (fusion_counts_first(size, o.fuseCount) && !count_cloud(r, size, countedDepths)) return false;
	Cloud cloud(size);
	if (size.capacity && !cloud.allocated()) {
		fprintf(stderr, "error: out of host memory for a cloud of up to %llu points\n", (unsigned long long)size.capacity);
		return false;
	}
	if (!fuse_cloud(r, cloud, size, countedDepths)) return false;
	const double tFused = now_s();
	if (o.verbosity > 1)
		printf("Depth-maps fused and filtered: %zu depth-maps, %llu depths, %llu points (%d%%) in %.2f s (%.2f Mpoints/s)\n", r.deal.fuseOrder.size(),
		       (unsigned long long)cloud.nDepths, (unsigned long long)cloud.nPoints, cloud.nDepths ? (int)std::lround(100.0 * cloud.nPoints / cloud.nDepths) : 0, tFused - r.tCopied,
		       cloud.nPoints / (tFused - r.tCopied) / 1e6);
	if (!save_cloud(r, cloud)) return false;
	if (!r.saver->wait_written()) return false;
	if (o.verbosity > 1) printf("Scene, point cloud and depth-maps saved (%.2f s after the fusion); total %.2f s\n", now_s() - tFused, now_s() - r.tStart);
	release_all(r);
	return true;
}

} // namespace

int main(int argc, char** argv) {
	const double tStart = now_s();
	Options o;
	std::string err;
	const ParseResult parsed = parse_options(argc, argv, o, err);
	for (const auto& note : o.notes) fprintf(stderr, "note: %s\n", note.c_str());
	if (parsed == PARSE_ERROR) { fprintf(stderr, "error: %s\n", err.c_str()); return EXIT_FAILURE; }
	if (parsed == PARSE_USAGE) { fputs(kUsage, stderr); return EXIT_FAILURE; }
	if (o.sampleMesh != 0) return run_sample_mesh(o);
	if (o.thFilterPointCloud < 0) return run_point_cloud_filter(o);

	Run r(o, tStart);
	start_contexts(r);
	if (!read_scene(r)) return EXIT_FAILURE;
	select_all_views(r);
	if (!contexts_ready(r)) return EXIT_FAILURE;
	list_todo(r);
	if (!deal_and_budget(r) || !resume_finished(r)) return EXIT_FAILURE;
	plan_image_batches(r);
	if (!load_images(r) || !rescale_neighbours(r) || !set_ignore_masks(r) || !load_depth_priors(r) || !set_prior_regions(r)) return EXIT_FAILURE;
	if (!start_saver_and_workers(r) || !run_outer_iterations(r) || !finish_estimates(r)) return EXIT_FAILURE;
	if (!filter_stage(r) || !final_maps_on_host(r)) return EXIT_FAILURE;
	if (o.fusionMode == 1 || r.todo.empty()) return finish_without_fusion(r) ? EXIT_SUCCESS : EXIT_FAILURE;
	return on_first_device(r, false, [&] { return fuse_and_save(r); }) ? EXIT_SUCCESS : EXIT_FAILURE;
}
