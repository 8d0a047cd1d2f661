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
 * that existing command lines keep their results; one device); optical flow, semantic priors and SGM modes are not available and
 * the corresponding flags are accepted and ignored with a note.
 *
 * How the run is laid out in time (the reference overlaps image k + 1's InitViews with image k's estimate, SceneDensify.cpp:3699-3703;
 * here the unit is a batch of reference images):
 *   load     all cores decode / resize the images and select the source views at the same time; uploads go out as images arrive
 *   estimate a loader thread prepares the initial maps of batch k + 1 (triangulation on all cores, upload) while the device
 *            estimates batch k; after the last outer iteration a copier thread brings finished batches back and a pool of writer
 *            threads saves the depth maps while the next batch is estimated and while the fusion runs
 *   resume   an image whose final depth map is already in the working folder is not estimated again (SceneDensify.cpp:3865-3880)
 */
#include "../../include/hcmvs_hip.h"
#include "ply_mesh.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

namespace {

struct Options { // DensifyPointCloud.cpp:139-198 (defaults from there)
	std::string input, output, workdir;
	std::string ignoreMaskLabel;  // --ignore-mask-label: labels of the segmentation image whose pixels are not estimated (empty: none)
	int resolutionLevel = 1, numberViews = 5, numberViewsFuse = 2, fusionMode = 0, verbosity = 2;
	int estimationIters = 1, estimationItersExternal = 4, adaptHalfWin = 5, propagateHalfWin = 1, propagateStep = 4;
	float photometricFlow = 0.5f, depthweight = 1.f, normalweight = 1.f;
	int initTriangulate = 1;      // 1: Delaunay init from the sparse points, 0: read the previous level's maps (SceneDensify.cpp:522-553)
	int minViewsTrustPoint = 2;   // < 2: splat the sparse points instead (SceneDensify.cpp:783-808)
	int fuseCount = -1;           // --fuse-count 0|1: fuse once with worst-case buffers / count first, then fuse with exact buffers (-1: count first when
	                              // the worst case exceeds 4 GiB)
	int fuseOrder = 0;            // hcmvs_set_fuse_order: 0 the reference's raster order (its cloud, point for point), 1 hashed order
	                              // (shorter dependence chains; point count within 1 % of the reference's)
	int estimateColors = 2, estimateNormals = 2;   // 2: during fusion, 1: after it (DepthMap.cpp:2125-2269), 0: none
	int maxResolution = 3200, minResolution = 640;  // DensifyPointCloud.cpp:144-145
	int nOptimize = 2;            // --n-nOptimize (DensifyPointCloud.cpp:164, 268): bits REMOVE_SPECKLES 1 | FILL_GAPS 2 (DepthMap.h:113-118) gate the fork's
	                              // RemoveSmallSegments + GapInterpolation after outer iterations 1 and 2 (SceneDensify.cpp:3916, 3939-3958)
	int postFilter = -1;          // --n-postfilter 0|1: override of that gate (-1: follow --n-nOptimize)
	int viewspread = 0;           // --n-viewspread 1: view spread (DepthMap.cpp:1504-1608).  The reference's default is 1; 0 here keeps
	                              // the results of every existing command line
	int postFilterInterleave = 0; // --n-postfilter-interleave 1: estimate(k) -> post-filter(k) -> estimate(k + 1), the reference's own order
	                              // (SceneDensify.cpp:3889-3965), one image per launch; 0: estimate all, then filter all
	int nFilter = 0;              // --n-filter 0|1|2: the depth-map filter stage before the fusion (Scene::DenseReconstructionFilter, SceneDensify.cpp:4100-4185, which the
	                              // fork switched off with if(0) at :3721): 0 off, 1 adjust (bFilterAdjust = 1), 2 strict.  --n-nOptimize bit 4 (ADJUST_FILTER) stays inert
	int resume = 1;               // skip-if-exists (SceneDensify.cpp:3865-3880): an image whose final depth map is already in the working folder is not estimated again
	int restoreHypothesis = 0;    // 1: the `restore` binary's extra last-sweep hypothesis from the previous level's maps
	                              // (restore/libs/MVS/DepthMap.cpp:1527-1549); needs the previous level's maps in the working folder
	int device = 0, batch = 32;   // reference images per launch: 32 is the measured optimum (profiles/r02_knobs.txt); lowered when HBM is short
	std::vector<int> devices;     // --devices 0,1,...: one context + host thread per entry; reference images sharded over them by their position in
	                              // the fusion order (k mod N); post-filters and fusion on the first (an ordinal may repeat: two contexts on one GPU)
	uint32_t seed = 1234;
};

struct Camera { double K[9], R[9], C[3]; };
struct ImageData {
	std::string name;
	uint32_t id = 0;
	int w = 0, h = 0;
	Camera cam;
	std::vector<uint8_t> bgr;   // working-resolution colour image (B,G,R)
	std::vector<float> gray;    // Types.inl:2354-2400 toGray, normalised
	bool valid = false;
	std::vector<uint32_t> points;               // sparse points seen (>= 2 views), Scene.cpp:568-569
	struct Nb { uint32_t id; uint32_t points; float scale, angle, area, score; };
	std::vector<Nb> neighbors;                  // Scene.cpp:640-650, sorted by score
	std::vector<uint32_t> srcs;                 // SceneDensify.cpp:362-367 (the ids the estimate is called with: resampled copies get ids of their own)
	std::vector<float> srcScale;                // per source view: 1 or the scale it is resampled by (ViewData::ScaleImage)
	std::vector<uint32_t> srcImages;            // the scene images behind srcs
	float dMin = 0, dMax = 0;
	int dev = 0;                                                    // index of the device context that estimates this image (--devices)
	float *dDepth = nullptr, *dNormal = nullptr, *dConf = nullptr; // device maps, on the owner's device
	float *gDepth = nullptr, *gNormal = nullptr, *gConf = nullptr; // the copy on the first device, where the post-filters and the fusion run (== d* when dev == 0)
	float *dHintDepth = nullptr, *dHintNormal = nullptr;            // previous level's maps, resized (restore variant)
};
struct Vertex { float X[3]; std::vector<std::pair<uint32_t, float>> views; };

// ---- .mvs (Interface.h:316-354 archive primitives) ----------------------------------------------------------------
struct Reader {
	std::ifstream f;
	template <typename T> T get() { T v; f.read((char*)&v, sizeof v); return v; }
	std::string str() { uint64_t n = get<uint64_t>(); std::string s(n, '\0'); if (n) f.read(&s[0], (std::streamsize)n); return s; }
	void mat(double* m, int n) { f.read((char*)m, sizeof(double) * n); }
};
struct MvsCamera { std::string name; uint32_t w, h; double K[9], R[9], C[3]; };
struct MvsPose { double R[9], C[3]; };
struct MvsPlatform { std::string name; std::vector<MvsCamera> cams; std::vector<MvsPose> poses; };
struct MvsImage { std::string name; uint32_t platformID, cameraID, poseID, ID; };

// normals / colors (optional): the vertices' normals (3 f32) and colours (B,G,R) that follow the vertices (Interface.h:607-609)
bool load_mvs(const std::string& path, std::vector<MvsPlatform>& platforms, std::vector<MvsImage>& images, std::vector<Vertex>& verts,
              std::vector<float>* normals = nullptr, std::vector<uint8_t>* colors = nullptr) {
	Reader r;
	r.f.open(path, std::ios::binary);
	if (!r.f) return false;
	char magic[4];
	r.f.read(magic, 4);
	if (strncmp(magic, "MVSI", 4) != 0) return false;
	const uint32_t ver = r.get<uint32_t>();
	r.get<uint32_t>();
	if (ver < 3 || ver > 5) { fprintf(stderr, "error: unsupported MVSI version %u\n", ver); return false; }
	platforms.resize(r.get<uint64_t>());
	for (auto& p : platforms) {
		p.name = r.str();
		p.cams.resize(r.get<uint64_t>());
		for (auto& c : p.cams) {
			c.name = r.str();
			if (ver > 3) r.str(); // bandName
			c.w = r.get<uint32_t>(); c.h = r.get<uint32_t>();
			r.mat(c.K, 9); r.mat(c.R, 9); r.mat(c.C, 3);
		}
		p.poses.resize(r.get<uint64_t>());
		for (auto& q : p.poses) { r.mat(q.R, 9); r.mat(q.C, 3); }
	}
	images.resize(r.get<uint64_t>());
	for (auto& im : images) {
		im.name = r.str();
		if (ver > 4) r.str(); // maskName
		im.platformID = r.get<uint32_t>(); im.cameraID = r.get<uint32_t>(); im.poseID = r.get<uint32_t>();
		im.ID = r.get<uint32_t>();
	}
	verts.resize(r.get<uint64_t>());
	for (auto& v : verts) {
		r.f.read((char*)v.X, 12);
		v.views.resize(r.get<uint64_t>());
		for (auto& w : v.views) { w.first = r.get<uint32_t>(); w.second = r.get<float>(); }
	}
	if (normals && colors) {
		const uint64_t nn = r.get<uint64_t>();
		if (!r.f || nn > verts.size()) return false;
		normals->resize(3 * nn);
		r.f.read((char*)normals->data(), (std::streamsize)(12 * nn));
		const uint64_t nc = r.get<uint64_t>();
		if (!r.f || nc > verts.size()) return false;
		colors->resize(3 * nc);
		r.f.read((char*)colors->data(), (std::streamsize)(3 * nc));
	}
	return (bool)r.f;
}

// the fused cloud's arrays: sized for the worst case before the fusion, filled by one copy from the device -- not
// value-initialised (a std::vector would touch gigabytes that are never used)
template <typename T>
struct RawArray {
	T* p = nullptr; size_t n = 0;
	explicit RawArray(size_t count) : p(count ? (T*)malloc(count * sizeof(T)) : nullptr), n(p ? count : 0) {}
	RawArray(const RawArray&) = delete;
	RawArray& operator=(const RawArray&) = delete;
	~RawArray() { free(p); }
	T* data() { return p; }
	const T* data() const { return p; }
	size_t size() const { return n; }
	void shrink(size_t count) { if (count < n) n = count; }
	void clear() { n = 0; }
	const T& operator[](size_t i) const { return p[i]; }
};

struct Writer { // binary output through one large buffer (a vertex is a handful of 4- and 8-byte fields)
	std::ofstream f;
	std::vector<char> buf;
	size_t fill = 0;
	Writer() : buf((size_t)32 << 20) {}
	void raw(const void* src, size_t bytes) {
		if (bytes > buf.size() - fill) { flush(); if (bytes > buf.size()) { f.write((const char*)src, (std::streamsize)bytes); return; } }
		memcpy(buf.data() + fill, src, bytes); fill += bytes;
	}
	void flush() { if (fill) f.write(buf.data(), (std::streamsize)fill); fill = 0; }
	template <typename T> void put(const T& v) { raw(&v, sizeof v); }
	void str(const std::string& s) { put<uint64_t>(s.size()); raw(s.data(), s.size()); }
};
bool save_mvs(const std::string& path, const std::vector<MvsPlatform>& platforms, const std::vector<MvsImage>& images,
              const RawArray<float>& xyz, const RawArray<float>& normals, const RawArray<uint8_t>& bgr,
              const RawArray<uint32_t>& nviews, const RawArray<uint32_t>& viewIds, const RawArray<float>& viewWeights) {
	Writer w;
	w.f.open(path, std::ios::binary);
	if (!w.f) return false;
	w.raw("MVSI", 4); w.put<uint32_t>(5); w.put<uint32_t>(0);
	w.put<uint64_t>(platforms.size());
	for (const auto& p : platforms) {
		w.str(p.name);
		w.put<uint64_t>(p.cams.size());
		for (const auto& c : p.cams) {
			w.str(c.name); w.str("");
			w.put(c.w); w.put(c.h);
			w.raw(c.K, 72); w.raw(c.R, 72); w.raw(c.C, 24);
		}
		w.put<uint64_t>(p.poses.size());
		for (const auto& q : p.poses) { w.raw(q.R, 72); w.raw(q.C, 24); }
	}
	w.put<uint64_t>(images.size());
	for (const auto& im : images) { w.str(im.name); w.str(""); w.put(im.platformID); w.put(im.cameraID); w.put(im.poseID); w.put(im.ID); }
	const uint64_t n = xyz.size() / 3;
	w.put<uint64_t>(n);
	uint64_t vo = 0;
	for (uint64_t i = 0; i < n; ++i) { // Interface::Vertex = X + views {imageID, confidence} (Interface.h:502-524; Scene.cpp:330-345 stores the weights as confidence)
		w.raw(&xyz[3 * i], 12);
		const uint64_t nv = i < nviews.size() ? nviews[i] : 0;
		w.put<uint64_t>(nv);
		for (uint64_t v = 0; v < nv; ++v) { w.put<uint32_t>(viewIds[vo + v]); w.put<float>(viewWeights[vo + v]); }
		vo += nv;
	}
	w.put<uint64_t>(normals.size() / 3); w.raw(normals.data(), normals.size() * 4);
	w.put<uint64_t>(bgr.size() / 3); w.raw(bgr.data(), bgr.size());
	for (int i = 0; i < 3; ++i) w.put<uint64_t>(0);
	const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
	w.raw(eye, sizeof eye);
	w.flush();
	return (bool)w.f;
}

// ---- images --------------------------------------------------------------------------------------------------------
// header of a binary PPM / PGM: size and channel count; the stream is left at the first pixel
bool pnm_header(std::ifstream& f, int& w, int& h, int& ch, int* maxvOut = nullptr) { // maxvOut: any maxval, reported
	std::string magic;
	f >> magic;
	if (magic != "P5" && magic != "P6") return false;
	auto next = [&]() { int v = 0; for (;;) { f >> std::ws; if (f.peek() == '#') { std::string l; std::getline(f, l); } else break; } f >> v; return v; };
	w = next(); h = next();
	const int maxv = next();
	f.get();
	ch = magic == "P6" ? 3 : 1;
	if (maxvOut) *maxvOut = maxv;
	return w > 0 && h > 0 && (maxv == 255 || maxvOut) && (bool)f;
}
// a label image of --ignore-mask-label as Image16U::Load reads it (Types.inl:2972-2991: imread UNCHANGED, colour -> gray, convertTo 16U):
// 8-bit P5, 16-bit P5 (maxval 65535, big-endian), or 8-bit P6 through cv::cvtColor's integer BGR2GRAY.  Any other maxval: no mask.
bool load_labels(const std::string& path, int& w, int& h, std::vector<uint16_t>& lab) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	int ch = 0, maxv = 0;
	if (!pnm_header(f, w, h, ch, &maxv)) return false;
	if (!(maxv == 255 || (maxv == 65535 && ch == 1))) return false;
	const size_t n = (size_t)w * h, bpp = maxv == 65535 ? 2 : 1;
	std::vector<uint8_t> raw(n * ch * bpp);
	f.read((char*)raw.data(), (std::streamsize)raw.size());
	if (!f) return false;
	lab.resize(n);
	for (size_t i = 0; i < n; ++i) {
		if (bpp == 2) lab[i] = (uint16_t)((raw[2 * i] << 8) | raw[2 * i + 1]);
		else if (ch == 1) lab[i] = raw[i];
		else lab[i] = (uint16_t)((raw[3 * i + 2] * 1868 + raw[3 * i + 1] * 9617 + raw[3 * i] * 4899 + 8192) >> 14); // file order R, G, B
	}
	return true;
}
bool pnm_size(const std::string& path, int& w, int& h) {
	std::ifstream f(path, std::ios::binary);
	int ch;
	return f && pnm_header(f, w, h, ch);
}
bool load_pnm(const std::string& path, int& w, int& h, std::vector<uint8_t>& bgr) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	int ch;
	if (!pnm_header(f, w, h, ch)) return false;
	std::vector<uint8_t> raw((size_t)w * h * ch);
	f.read((char*)raw.data(), (std::streamsize)raw.size());
	if (!f) return false;
	bgr.resize((size_t)w * h * 3);
	for (size_t i = 0; i < (size_t)w * h; ++i) {
		if (ch == 3) { bgr[3 * i] = raw[3 * i + 2]; bgr[3 * i + 1] = raw[3 * i + 1]; bgr[3 * i + 2] = raw[3 * i]; }
		else bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = raw[i];
	}
	return true;
}
// cv::resize(image, image, Size(nw, nh), 0, 0, INTER_AREA) on an 8-bit BGR image, as Image::ResizeImage calls it
// (Image.cpp:140-160), restated from OpenCV's published algorithm (imgproc/src/resize.cpp): an exact factor of 2 averages
// 2x2 blocks with (sum + 2) >> 2; another integer factor multiplies the block sum by 1/area and rounds; any other factor goes
// through computeResizeAreaTab / ResizeArea_Invoker in float and rounds (saturate_cast<uchar> = round half to even)
void resize_area_bgr(int& w, int& h, std::vector<uint8_t>& bgr, int nw, int nh) {
	std::vector<uint8_t> out((size_t)nw * nh * 3);
	const double sx = (double)w / nw, sy = (double)h / nh;
	const int ix = (int)sx, iy = (int)sy;
	auto rnd = [](float v) { const long r = lrintf(v); return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r)); };
	if ((double)ix == sx && (double)iy == sy) {
		const float inv = 1.f / (float)(ix * iy);
		for (int y = 0; y < nh; ++y)
			for (int x = 0; x < nw; ++x)
				for (int c = 0; c < 3; ++c) {
					int s = 0;
					for (int j = 0; j < iy; ++j)
						for (int i = 0; i < ix; ++i) s += bgr[3 * ((size_t)(y * iy + j) * w + (x * ix + i)) + c];
					out[3 * ((size_t)y * nw + x) + c] = (ix == 2 && iy == 2) ? (uint8_t)((s + 2) >> 2) : rnd((float)s * inv);
				}
	} else {
		struct Tab { std::vector<int> idx; std::vector<float> a; };
		auto cell = [](int d, double scale, int ssize, Tab& t) {
			t.idx.clear(); t.a.clear();
			const double f1 = d * scale, f2 = f1 + scale, cw = std::min(scale, ssize - f1);
			int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
			s2 = std::min(s2, ssize - 1); s1 = std::min(s1, s2);
			if (s1 - f1 > 1e-3) { t.idx.push_back(s1 - 1); t.a.push_back((float)((s1 - f1) / cw)); }
			for (int q = s1; q < s2; ++q) { t.idx.push_back(q); t.a.push_back((float)(1.0 / cw)); }
			if (f2 - s2 > 1e-3) { t.idx.push_back(s2); t.a.push_back((float)(std::min(std::min(f2 - s2, 1.), cw) / cw)); }
		};
		std::vector<Tab> xt((size_t)nw);
		for (int x = 0; x < nw; ++x) cell(x, sx, w, xt[x]);
#pragma omp parallel for schedule(static)
		for (int y = 0; y < nh; ++y) {
			Tab yt;
			cell(y, sy, h, yt);
			for (int x = 0; x < nw; ++x)
				for (int c = 0; c < 3; ++c) {
					float sum = 0.f;
					for (size_t j = 0; j < yt.idx.size(); ++j) {
						float buf = 0.f;
						for (size_t i = 0; i < xt[x].idx.size(); ++i) buf += (float)bgr[3 * ((size_t)yt.idx[j] * w + xt[x].idx[i]) + c] * xt[x].a[i];
						sum = j == 0 ? yt.a[j] * buf : sum + yt.a[j] * buf;
					}
					out[3 * ((size_t)y * nw + x) + c] = rnd(sum);
				}
		}
	}
	w = nw; h = nh; bgr.swap(out);
}
// TImage::computeMaxResolution (Types.inl:2442-2460) + Image::ResizeImage (Image.cpp:140-160): the working size of an image
void working_size(int w, int h, unsigned level, unsigned minSize, unsigned maxSize, int& nw, int& nh) {
	const unsigned imageSize = (unsigned)std::max(w, h);
	unsigned size;
	if (level == 0) size = std::min(imageSize, maxSize);
	else {
		size = imageSize >> level;
		if (size < minSize) { level = 0; while ((imageSize >> (level + 1)) >= minSize) ++level; size = imageSize >> level; }
		size = std::min(size, maxSize);
	}
	nw = w; nh = h;
	if (size == 0 || imageSize <= size) return;
	if (w > h) { nh = (int)((unsigned)h * size / (unsigned)w); nw = (int)size; }
	else { nw = (int)((unsigned)w * size / (unsigned)h); nh = (int)size; }
}

// ---- camera helpers (Camera.h) -------------------------------------------------------------------------------------
void mat3mul(const double* a, const double* b, double* c) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j]; c[i * 3 + j] = s; }
}
void w2c(const Camera& c, const float* X, double* o) {
	const double d[3] = {X[0] - c.C[0], X[1] - c.C[1], X[2] - c.C[2]};
	for (int i = 0; i < 3; ++i) o[i] = c.R[i * 3] * d[0] + c.R[i * 3 + 1] * d[1] + c.R[i * 3 + 2] * d[2];
}
// the camera of an image at the size w x h: Interface.h:451-459 pose composition (R = Rcam Rpose, C = Rpose^T Ccam + Cpose) and
// Scene.cpp:83-91 + Camera.h:167-180 (GetK): K normalised by max(w,h) of the camera, scaled to w x h
void image_camera(const MvsCamera& c, const MvsPose& q, int w, int h, Camera& cam) {
	mat3mul(c.R, q.R, cam.R);
	for (int k = 0; k < 3; ++k) cam.C[k] = q.R[0 * 3 + k] * c.C[0] + q.R[1 * 3 + k] * c.C[1] + q.R[2 * 3 + k] * c.C[2] + q.C[k];
	const double s = (double)std::max(w, h) / (c.w && c.h ? (double)std::max(c.w, c.h) : 1.0);
	memcpy(cam.K, c.K, sizeof cam.K);
	cam.K[1] = 0;
	cam.K[0] *= s; cam.K[4] *= s;
	if (c.K[2] == 0 && c.K[5] == 0) { cam.K[2] = 0.5 * (w - 1); cam.K[5] = 0.5 * (h - 1); }
	else { cam.K[2] *= s; cam.K[5] *= s; }
}
bool project(const Camera& c, const float* X, float& u, float& v, double& z) {
	double p[3];
	w2c(c, X, p);
	z = p[2];
	if (p[2] <= 0) return false;
	u = (float)(c.K[2] + c.K[0] * p[0] / p[2]); v = (float)(c.K[5] + c.K[4] * p[1] / p[2]);
	return true;
}

// Scene.cpp:545-661 SelectNeighborViews + Scene.cpp:665-678 FilterNeighborViews (defaults DepthMap.cpp:69-143)
bool select_views(std::vector<ImageData>& images, const std::vector<Vertex>& verts, uint32_t ID, int nMaxViews, int numberViews) {
	ImageData& A = images[ID];
	const float fOptimAngle = 10.f * 3.14159265f / 180.f, fMinAngle = 3.f * 3.14159265f / 180.f, fMaxAngle = 65.f * 3.14159265f / 180.f;
	struct Score { float score = 0, avgScale = 0, avgAngle = 0; uint32_t points = 0; };
	std::vector<Score> scores(images.size());
	for (uint32_t idx = 0; idx < verts.size(); ++idx) {
		const Vertex& v = verts[idx];
		bool seen = false;
		for (const auto& w : v.views) if (w.first == ID) { seen = true; break; }
		if (!seen) continue;
		if (v.views.size() >= 2) A.points.push_back(idx);
		double pc[3];
		w2c(A.cam, v.X, pc);
		const float V1[3] = {(float)(A.cam.C[0] - v.X[0]), (float)(A.cam.C[1] - v.X[1]), (float)(A.cam.C[2] - v.X[2])};
		const float fp1 = (float)(A.cam.K[0] / pc[2]); // Footprint, Scene.cpp:531-539
		for (const auto& w : v.views) {
			if (w.first == ID || w.first >= images.size() || !images[w.first].valid) continue;
			const ImageData& B = images[w.first];
			const float V2[3] = {(float)(B.cam.C[0] - v.X[0]), (float)(B.cam.C[1] - v.X[1]), (float)(B.cam.C[2] - v.X[2])};
			float ca = (V1[0] * V2[0] + V1[1] * V2[1] + V1[2] * V2[2]) /
			           std::sqrt((V1[0] * V1[0] + V1[1] * V1[1] + V1[2] * V1[2]) * (V2[0] * V2[0] + V2[1] * V2[1] + V2[2] * V2[2]));
			ca = std::min(1.f, std::max(-1.f, ca));
			const float ang = std::acos(ca);
			const float wAngle = std::min(std::pow(ang / fOptimAngle, 1.5f), 1.f);
			double pb[3];
			w2c(B.cam, v.X, pb);
			const float r = fp1 / (float)(B.cam.K[0] / pb[2]);
			const float wScale = r > 1.6f ? (1.6f / r) * (1.6f / r) : (r >= 1.f ? 1.f : r * r);
			Score& s = scores[w.first];
			s.score += wAngle * wScale; s.avgScale += r; s.avgAngle += ang; ++s.points;
		}
	}
	for (uint32_t IDB = 0; IDB < images.size(); ++IDB) {
		const Score& s = scores[IDB];
		if (!images[IDB].valid || s.points < 3) continue;
		const ImageData& B = images[IDB];
		bool grid[16][16] = {};
		int n = 0;
		for (uint32_t idx : A.points) {
			const Vertex& v = verts[idx];
			bool inB = false;
			for (const auto& w : v.views) if (w.first == IDB) { inB = true; break; }
			if (!inB) continue;
			float ua, va, ub, vb; double za, zb;
			if (!project(A.cam, v.X, ua, va, za) || !project(B.cam, v.X, ub, vb, zb)) continue;
			if (ua < 0 || va < 0 || ua >= A.w || va >= A.h || ub < 0 || vb < 0 || ub >= B.w || vb >= B.h) continue;
			grid[std::min(15, (int)(ua / A.w * 16))][std::min(15, (int)(va / A.h * 16))] = true; // Util.inl:711-730
			++n;
		}
		if (!n) continue;
		int cells = 0;
		for (auto& row : grid) for (bool c : row) cells += c;
		ImageData::Nb nb{IDB, s.points, s.avgScale / s.points, s.avgAngle / s.points, cells / 256.f, 0.f};
		nb.score = s.score * nb.area;
		A.neighbors.push_back(nb);
	}
	std::stable_sort(A.neighbors.begin(), A.neighbors.end(), [](const ImageData::Nb& a, const ImageData::Nb& b) { return a.score > b.score; });
	if (A.points.size() <= 3 || A.neighbors.size() < (size_t)std::min<int>(2, (int)images.size() - 1)) return false;
	std::vector<ImageData::Nb> kept;
	for (const auto& nb : A.neighbors)
		if (!(nb.area < 0.01f) && nb.scale >= 0.2f && nb.scale < 3.2f && nb.angle >= fMinAngle && nb.angle < fMaxAngle) kept.push_back(nb);
	if ((int)kept.size() > nMaxViews) kept.resize(nMaxViews);
	A.neighbors.swap(kept);
	if (A.neighbors.empty()) return false;
	// SceneDensify.cpp:362-367: neighbours in score order while #images <= number-views and score >= best * 0.03
	const float fMinScore = A.neighbors[0].score * (0.3f * 0.1f);
	for (const auto& nb : A.neighbors) {
		if ((numberViews && (int)A.srcs.size() + 1 > numberViews) || nb.score < fMinScore) break;
		A.srcs.push_back(nb.id);
		A.srcScale.push_back(std::fabs(nb.scale - 1.f) >= 0.15f ? nb.scale : 1.f); // >= 15 %: the view is resampled (DepthMap.h:233-238)
	}
	return !A.srcs.empty();
}

// raw 'DR' file (Interface.h:634-652): any of depth (flag 1), normal (2), confidence (4); null = not stored
bool save_dmap(const std::string& path, const ImageData& im, const float* d, const float* n, const float* c) {
	std::ofstream f(path + ".tmp", std::ios::binary); // atomic like DepthData::Save (DepthMap.cpp:253-286)
	if (!f) return false;
	struct __attribute__((packed)) Hdr { uint16_t name; uint8_t type, pad; uint32_t iw, ih, dw, dh; float dMin, dMax; } h;
	const size_t px = (size_t)im.w * im.h;
	h.name = 0x5244; h.type = (uint8_t)((d ? 1 : 0) | (n ? 2 : 0) | (c ? 4 : 0)); h.pad = 0; h.iw = h.dw = (uint32_t)im.w; h.ih = h.dh = (uint32_t)im.h; h.dMin = im.dMin; h.dMax = im.dMax;
	f.write((const char*)&h, 28);
	const uint16_t nl = (uint16_t)im.name.size();
	f.write((const char*)&nl, 2); f.write(im.name.data(), nl);
	const std::vector<uint32_t>& ids = im.srcImages.empty() ? im.srcs : im.srcImages; // scene image ids, not the ids of resampled copies
	const uint32_t nids = 1 + (uint32_t)ids.size();
	f.write((const char*)&nids, 4); f.write((const char*)&im.id, 4); f.write((const char*)ids.data(), (std::streamsize)ids.size() * 4);
	f.write((const char*)im.cam.K, 72); f.write((const char*)im.cam.R, 72); f.write((const char*)im.cam.C, 24);
	if (d) f.write((const char*)d, (std::streamsize)px * 4);
	if (n) f.write((const char*)n, (std::streamsize)px * 12);
	if (c) f.write((const char*)c, (std::streamsize)px * 4);
	f.close();
	return (bool)f && std::rename((path + ".tmp").c_str(), path.c_str()) == 0;
}
bool save_ply(const std::string& path, const RawArray<float>& xyz, const RawArray<float>& nrm, const RawArray<uint8_t>& bgr) {
	Writer w;
	w.f.open(path, std::ios::binary); // PointCloud.cpp:189-240
	if (!w.f) return false;
	std::ostringstream f;
	const size_t n = xyz.size() / 3;
	const bool hasN = nrm.size() == xyz.size() && n > 0, hasC = bgr.size() == xyz.size() && n > 0; // PointCloud.cpp:105-128: only what exists
	f << "ply\nformat binary_little_endian 1.0\nelement vertex " << n << "\nproperty float x\nproperty float y\nproperty float z\n";
	if (hasN) f << "property float nx\nproperty float ny\nproperty float nz\n";
	if (hasC) f << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
	f << "end_header\n";
	w.raw(f.str().data(), f.str().size());
	for (size_t i = 0; i < n; ++i) {
		w.raw(&xyz[3 * i], 12);
		if (hasN) w.raw(&nrm[3 * i], 12);
		if (hasC) { const uint8_t rgb[3] = {bgr[3 * i + 2], bgr[3 * i + 1], bgr[3 * i]}; w.raw(rgb, 3); }
	}
	w.flush();
	return (bool)w.f;
}

// raw 'DR' depth map written by save_dmap / the reference (Interface.h:634-652); returns false when absent or malformed
struct DmapFile { int w = 0, h = 0; float dMin = 0, dMax = 0; std::vector<float> d, n, c; };
// what: bit 1 depth, 2 normal, 4 confidence -- the maps wanted; a wanted map the file does not hold fails the load.
// headerOnly: size and range only
bool load_dmap(const std::string& path, DmapFile& m, int what, bool headerOnly = false) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	struct __attribute__((packed)) Hdr { uint16_t name; uint8_t type, pad; uint32_t iw, ih, dw, dh; float dMin, dMax; } hd;
	f.read((char*)&hd, 28);
	if (!f || hd.name != 0x5244 || (hd.type & what) != what) return false;
	m.w = (int)hd.dw; m.h = (int)hd.dh; m.dMin = hd.dMin; m.dMax = hd.dMax;
	if (m.w <= 0 || m.h <= 0 || m.w > 65536 || m.h > 65536) return false;
	if (headerOnly) return true;
	uint16_t nl = 0; f.read((char*)&nl, 2); f.seekg(nl, std::ios::cur);
	uint32_t nids = 0; f.read((char*)&nids, 4); f.seekg((std::streamoff)nids * 4 + 72 + 72 + 24, std::ios::cur);
	const size_t px = (size_t)m.w * m.h;
	auto part = [&](int bit, size_t floats, std::vector<float>& v) {
		if (!(hd.type & bit)) return;
		if (what & bit) { v.resize(floats); f.read((char*)v.data(), (std::streamsize)floats * 4); }
		else f.seekg((std::streamoff)floats * 4, std::ios::cur);
	};
	part(1, px, m.d); part(2, px * 3, m.n); part(4, px, m.c);
	return (bool)f;
}
// cv::resize(..., INTER_CUBIC) as the hand-off uses it (SceneDensify.cpp:541-542): Keys kernel a = -0.75, pixel centres
// aligned ((x + 0.5) * scale - 0.5), replicated border
void resize_cubic(const std::vector<float>& src, int sw, int sh, int ch, std::vector<float>& dst, int dw, int dh) {
	dst.resize((size_t)dw * dh * ch);
	auto weights = [](float t, float* w) {
		const float A = -0.75f;
		w[0] = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A;
		w[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
		w[2] = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1;
		w[3] = 1.f - w[0] - w[1] - w[2];
	};
	const double sx = (double)sw / dw, sy = (double)sh / dh;
	for (int y = 0; y < dh; ++y) {
		const float fy = (float)((y + 0.5) * sy - 0.5);
		const int iy = (int)std::floor(fy);
		float wy[4]; weights(fy - iy, wy);
		for (int x = 0; x < dw; ++x) {
			const float fx = (float)((x + 0.5) * sx - 0.5);
			const int ix = (int)std::floor(fx);
			float wx[4]; weights(fx - ix, wx);
			for (int c = 0; c < ch; ++c) {
				float acc = 0.f;
				for (int j = 0; j < 4; ++j) {
					const int yy = std::min(std::max(iy - 1 + j, 0), sh - 1);
					float row = 0.f;
					for (int i = 0; i < 4; ++i) {
						const int xx = std::min(std::max(ix - 1 + i, 0), sw - 1);
						row += wx[i] * src[((size_t)yy * sw + xx) * ch + c];
					}
					acc += wy[j] * row;
				}
				dst[((size_t)y * dw + x) * ch + c] = acc;
			}
		}
	}
}

std::string dirname_of(const std::string& p) { const size_t k = p.find_last_of('/'); return k == std::string::npos ? "." : p.substr(0, k); }

} // namespace

#define CHK(call) do { const int rc_ = (call); if (rc_ != HCMVS_OK) { fprintf(stderr, "error: %s -> %d (%s)\n", #call, rc_, hcmvs_last_error(ctx)); return EXIT_FAILURE; } } while (0)
#define HIPOK(call) do { if ((call) != hipSuccess) { fprintf(stderr, "error: %s failed\n", #call); return EXIT_FAILURE; } } while (0)

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::string map_path(const std::string& dir, const char* fmt, uint32_t id) { char nm[96]; snprintf(nm, sizeof nm, fmt, id); return dir + nm; }

namespace {

// One batch of reference images whose initial maps the loader thread prepares while the device works on the batch before it
// (the reference requests "next image initialization to be performed while computing this depth-map", SceneDensify.cpp:3699-3703)
struct Prepared { bool ready = false; int failed = 0; uint32_t failedId = 0; };

// the initial maps of one image (SceneDensify.cpp:772-812) and, for the `restore` variant, its hint maps: host part
struct InitMaps { std::vector<float> d, n, hd, hn; int failed = 0; };

// Saving the final maps: a copier thread brings the maps of finished batches to the host (its own stream; the device keeps
// estimating), writer threads put them on disk.  The fusion mutates the depth maps (SceneDensify.cpp:3447-3449), so it waits for
// the copies -- not for the files.
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
struct Saver {
	std::mutex mu; std::condition_variable cv;
	std::deque<uint32_t> toCopy; std::deque<std::unique_ptr<SaveJob>> toWrite;
	size_t bytesQueued = 0, copied = 0, written = 0, submitted = 0;
	bool closing = false; std::string error;
	static constexpr size_t kMaxQueuedBytes = (size_t)12 << 30; // host memory the copier may run ahead of the writers
};

// --filter-point-cloud < 0 (DensifyPointCloud.cpp:399-414): Scene::Load, Scene::PointCloudFilter(th) on the first device of --devices,
// then <output base>_filtered.mvs / .ply; no densify runs.  The cameras are taken at their own resolution and no image is opened, except
// the header of an image whose camera has no resolution (Scene::LoadInterface reads the size from the image then).
int run_point_cloud_filter(const Options& o, int th) {
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
int run_sample_mesh(const Options& o, float sample, unsigned long long seed) {
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

} // namespace

int main(int argc, char** argv) {
	const double tStart = now_s();
	Options o;
	std::map<std::string, std::string> kv;
	// every option of the reference's table (DensifyPointCloud.cpp:71-198) plus the ones of this driver; all take a value.
	// Unknown options are an error (boost::program_options throws on them, DensifyPointCloud.cpp:222-233).
	static const char* const kKnown[] = {
		"-i", "--input-file", "-o", "--output-file", "-w", "--working-folder", "-c", "--config-file", "--dense-config-file", "--archive-type",
		"--process-priority", "--max-threads", "-v", "--verbosity", "--resolution-level", "--max-resolution", "--min-resolution",
		"--number-views", "--number-views-fuse", "--ignore-mask-label", "--use-semantic", "--estimate-colors", "--estimate-normals",
		"--sample-mesh", "--filter-point-cloud", "--fusion-mode", "--depthweight", "--normalweight", "--semantic-multiplier",
		"--sigma-texture", "--sigma-prior", "--ransac-epsilon", "--n-nOptimize", "--ransac-cluster", "--ransac-min-points",
		"--project-labels", "--ransac-probability", "--n-EstimationIters", "--n-EstimationIters-external", "--n-photo2geo",
		"--n-txthreshold", "--n-maxgeo_proportion", "--n-para_part", "--n-para_part2", "--n-txthreshold2", "--n-para_tapa",
		"--n-para_tapa2", "--n-para_prior", "--n-para_prior2", "--n-photometric_flow", "--n-usepartconsistency",
		"--n-usegeoconsistency", "--n-initTriangulate", "--n-viewspread", "--n-opticalflow", "--n-adapthalfwin",
		"--n-propagatehalfwin", "--n-propagatestep",
		// this driver's own
		"--min-views-trust-point", "--fuse-order", "--fuse-count", "--device", "--devices", "--batch", "--seed", "--restore-hypothesis", "--n-postfilter", "--n-postfilter-interleave", "--resume", "--n-filter"};
	for (int i = 1; i < argc; ++i) {
		std::string a = argv[i], val;
		if (a == "-h" || a == "--help") { kv["--help"] = "1"; continue; }
		const size_t eq = a.find('=');
		bool haveVal = false;
		if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); haveVal = true; }
		bool known = false;
		for (const char* k : kKnown) known = known || a == k;
		if (!known) { fprintf(stderr, "error: unrecognised option '%s'\n", a.c_str()); return EXIT_FAILURE; }
		if (!haveVal) { // the value is the next argument, whatever it starts with (negative numbers are values)
			if (i + 1 >= argc) { fprintf(stderr, "error: the required argument for option '%s' is missing\n", a.c_str()); return EXIT_FAILURE; }
			val = argv[++i];
		}
		kv[a] = val;
	}
	auto geti = [&](const char* k, int& v) { if (kv.count(k)) v = atoi(kv[k].c_str()); };
	auto getf = [&](const char* k, float& v) { if (kv.count(k)) v = (float)atof(kv[k].c_str()); };
	for (const char* k : {"-i", "--input-file"}) if (kv.count(k)) o.input = kv[k];
	for (const char* k : {"-o", "--output-file"}) if (kv.count(k)) o.output = kv[k];
	for (const char* k : {"-w", "--working-folder"}) if (kv.count(k)) o.workdir = kv[k];
	geti("-v", o.verbosity); geti("--verbosity", o.verbosity);
	if (kv.count("--ignore-mask-label")) o.ignoreMaskLabel = kv["--ignore-mask-label"];
	geti("--resolution-level", o.resolutionLevel); geti("--number-views", o.numberViews); geti("--number-views-fuse", o.numberViewsFuse);
	geti("--fusion-mode", o.fusionMode); geti("--n-EstimationIters", o.estimationIters);
	geti("--n-EstimationIters-external", o.estimationItersExternal); geti("--n-adapthalfwin", o.adaptHalfWin);
	geti("--n-propagatehalfwin", o.propagateHalfWin); geti("--n-propagatestep", o.propagateStep);
	getf("--n-photometric_flow", o.photometricFlow); getf("--depthweight", o.depthweight); getf("--normalweight", o.normalweight);
	geti("--n-initTriangulate", o.initTriangulate); geti("--min-views-trust-point", o.minViewsTrustPoint);
	geti("--fuse-order", o.fuseOrder); geti("--fuse-count", o.fuseCount); geti("--restore-hypothesis", o.restoreHypothesis); geti("--n-postfilter", o.postFilter); geti("--n-postfilter-interleave", o.postFilterInterleave); geti("--n-nOptimize", o.nOptimize); geti("--resume", o.resume); geti("--n-viewspread", o.viewspread); geti("--n-filter", o.nFilter);
	geti("--device", o.device); geti("--batch", o.batch);
	if (kv.count("--devices")) { // comma-separated HIP ordinals
		std::stringstream ss(kv["--devices"]);
		std::string tok;
		while (std::getline(ss, tok, ',')) {
			if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "error: --devices expects a comma-separated list of device ordinals\n"); return EXIT_FAILURE; }
			o.devices.push_back(atoi(tok.c_str()));
		}
		if (o.devices.empty() || o.devices.size() > 64) { fprintf(stderr, "error: --devices expects 1 to 64 device ordinals\n"); return EXIT_FAILURE; }
	} else o.devices.push_back(o.device);
	o.device = o.devices[0];
	if (kv.count("--seed")) o.seed = (uint32_t)strtoul(kv["--seed"].c_str(), nullptr, 10);
	geti("--estimate-colors", o.estimateColors); geti("--estimate-normals", o.estimateNormals);
	geti("--max-resolution", o.maxResolution); geti("--min-resolution", o.minResolution);
	if (o.postFilter < 0) o.postFilter = (o.nOptimize & 3) != 0 ? 1 : 0; // OPTDENSE::OPTIMIZE = REMOVE_SPECKLES | FILL_GAPS (DepthMap.h:113-118)
	for (const char* k : {"--n-opticalflow", "--use-semantic", "--n-usegeoconsistency", "--n-usepartconsistency"})
		if (kv.count(k) && atoi(kv[k].c_str()) != 0 && o.verbosity > 1)
			fprintf(stderr, "note: %s is not available in this build (defined subset); treated as 0\n", k);
	const int thFilterPointCloud = kv.count("--filter-point-cloud") ? atoi(kv["--filter-point-cloud"].c_str()) : 0; // >= 0: no effect, as in the reference
	const float sampleMesh = kv.count("--sample-mesh") ? (float)atof(kv["--sample-mesh"].c_str()) : 0.f; // 0: no effect, as in the reference
	if (o.input.empty() || kv.count("--help")) {
		fprintf(stderr, "usage: DensifyPointCloud -i scene.mvs [-o out.mvs] [-w dir] [--resolution-level n] [--number-views n] "
		                "[--n-EstimationIters n] [--n-EstimationIters-external n] [--n-adapthalfwin n] [--fusion-mode 0|1] ...\n"
		                "       --n-viewspread 0|1   from outer iteration 1 on every pixel also tries what its source views' depth maps hold where it projects to\n"
		                "                            (default 0; the reference's default is 1 -- 0 keeps the results of command lines written before it existed)\n"
		                "       --n-filter 0|1|2     the depth-map filter stage before the fusion: every depth map against up to 8 neighbours' maps (0 off, the default;\n"
		                "                            1 adjust: consistent depths are averaged, 2 strict: kept as they are); the final .dmap files hold the filtered maps\n"
		                "                            (with --resume 1 a second run loads those filtered maps and filters them again, as the reference would)\n"
		                "       DensifyPointCloud -i dense.mvs [-o out.mvs] --filter-point-cloud <negative threshold>   (visibility filter of the cloud only:\n"
		                "       writes <out>_filtered.mvs and <out>_filtered.ply)\n"
		                "       DensifyPointCloud -i mesh.ply [-o out.mvs] --sample-mesh <d> [--seed n]   (samples a point cloud on a PLY triangle mesh and writes\n"
		                "       <out>.ply: d > 0 points per square unit, d < 0 minus the number of points; colours when the mesh is textured by a binary PPM)\n");
		return EXIT_FAILURE;
	}
	if (o.workdir.empty()) o.workdir = dirname_of(o.input);
	if (o.output.empty()) o.output = o.input.substr(0, o.input.rfind('.')) + "_dense.mvs";
	if (sampleMesh != 0) return run_sample_mesh(o, sampleMesh, kv.count("--seed") ? strtoull(kv["--seed"].c_str(), nullptr, 10) : (unsigned long long)o.seed);
	if (thFilterPointCloud < 0) return run_point_cloud_filter(o, thFilterPointCloud);
	if (o.fusionMode < 0) { fprintf(stderr, "error: SGM fusion modes are not available\n"); return EXIT_FAILURE; }
	if (o.nFilter < 0 || o.nFilter > 2) { fprintf(stderr, "error: --n-filter expects 0 (off), 1 (adjust) or 2 (strict)\n"); return EXIT_FAILURE; }
	if (o.batch < 1) o.batch = 1;
	if (o.batch > HCMVS_MAX_BATCH) o.batch = HCMVS_MAX_BATCH;
	if (o.estimationItersExternal < 1) o.estimationItersExternal = 1;

	// the device contexts come up (HIP runtime start, ~0.4 s) while the scene is read and the views are selected on the host.
	// One context and, later, one host thread per entry of --devices; devs[0] is where the post-filters and the fusion run.
	struct DeviceCtx { int ordinal = 0; hcmvs_ctx* ctx = nullptr; int createRc = HCMVS_OK; std::mutex upMu; std::vector<uint32_t> work; };
	std::vector<DeviceCtx> devs(o.devices.size());
	for (size_t d = 0; d < devs.size(); ++d) devs[d].ordinal = o.devices[d];
	const int nDev = (int)devs.size();
	std::thread createThread([&] { for (auto& d : devs) d.createRc = hcmvs_create(d.ordinal, &d.ctx); });
	struct CreateJoin { std::thread& t; ~CreateJoin() { if (t.joinable()) t.join(); } } createJoin{createThread};
	std::vector<MvsPlatform> platforms; std::vector<MvsImage> mimages; std::vector<Vertex> verts;
	if (!load_mvs(o.input, platforms, mimages, verts)) { fprintf(stderr, "error: can not load '%s'\n", o.input.c_str()); return EXIT_FAILURE; }
	std::vector<ImageData> images(mimages.size());
	std::vector<std::string> paths(mimages.size());
	unsigned nValid = 0;
	// headers first: the working size and the camera of every image are known before a pixel is decoded, which is all the view
	// selection needs
	for (size_t i = 0; i < mimages.size(); ++i) {
		ImageData& im = images[i];
		im.name = mimages[i].name; im.id = (uint32_t)i;
		if (mimages[i].poseID == 0xFFFFFFFFu || mimages[i].platformID >= platforms.size()) continue; // uncalibrated
		const MvsPlatform& p = platforms[mimages[i].platformID];
		const MvsCamera& c = p.cams[mimages[i].cameraID];
		const MvsPose& q = p.poses[mimages[i].poseID];
		paths[i] = im.name[0] == '/' ? im.name : dirname_of(o.input) + "/" + im.name;
		int fw = 0, fh = 0;
		if (!pnm_size(paths[i], fw, fh)) { fprintf(stderr, "error: failed loading image '%s' (binary PPM/PGM expected)\n", paths[i].c_str()); return EXIT_FAILURE; }
		// SceneDensify.cpp:3612-3615: one INTER_AREA resize to the resolution level's size, within [min-resolution, max-resolution]
		working_size(fw, fh, (unsigned)std::max(0, o.resolutionLevel), (unsigned)std::max(1, o.minResolution), (unsigned)std::max(1, o.maxResolution), im.w, im.h);
		image_camera(c, q, im.w, im.h, im.cam); // K rescaled to the working resolution
		im.valid = true;
		++nValid;
	}
	// the view selection of every image, all cores (every image writes only its own lists; the selection reads cameras and sizes,
	// no pixels; SceneDensify.cpp:3590-3634 is an OpenMP loop too)
	std::vector<char> selected(images.size(), 0);
#pragma omp parallel for schedule(dynamic, 1)
	for (long i = 0; i < (long)images.size(); ++i)
		if (images[i].valid) selected[i] = select_views(images, verts, (uint32_t)i, 12, o.numberViews) ? 1 : 0;
	// decode + resize + gray conversion of the images on all cores; an image goes to the device as soon as it is decoded.  Runs
	// AFTER the loader thread below has started: the triangulated initial maps need cameras and sparse points only, so the first
	// batch's initialisation overlaps the decoding.
	std::string loadError;
	std::mutex errMu;
	// which device needs the gray image of which scene image (its own reference images and their source views); filled in once the
	// images are assigned to the devices, before load_images() runs.  The first device also gets camera + colour image of every
	// other image (a fuse-only view: hcmvs_upload_view with gray = NULL), because it filters and fuses the whole scene.
	std::vector<std::vector<char>> needGray(devs.size(), std::vector<char>(images.size(), 1));
	auto load_images = [&]() {
		const long N = (long)images.size();
#pragma omp parallel for schedule(dynamic, 1)
		for (long t = 0; t < N; ++t) {
			ImageData& im = images[t];
			if (!im.valid) continue;
			int fw = 0, fh = 0;
			std::vector<uint8_t> bgr;
			if (!load_pnm(paths[t], fw, fh, bgr)) { std::lock_guard<std::mutex> g(errMu); loadError = "failed loading image '" + paths[t] + "'"; continue; }
			if (fw != im.w || fh != im.h) resize_area_bgr(fw, fh, bgr, im.w, im.h);
			// gray and colour image go into page-locked memory of this thread: what is left for the (serial) upload is the transfer
			static thread_local struct Pinned { char* p = nullptr; size_t cap = 0; } pin; // lives as long as its thread; the process ends with them
			const size_t px = (size_t)im.w * im.h, need = px * 4 + px * 3;
			if (pin.cap < need) {
				if (pin.p) (void)hipHostFree(pin.p);
				pin.p = nullptr; pin.cap = 0;
				if (hipSetDevice(o.device) == hipSuccess && hipHostMalloc((void**)&pin.p, need, hipHostMallocPortable) == hipSuccess) pin.cap = need;
				else { (void)hipGetLastError(); pin.p = nullptr; }
			}
			std::vector<float> grayVec;
			float* gray = (float*)pin.p;
			uint8_t* bgrUp = pin.p ? (uint8_t*)(pin.p + px * 4) : bgr.data();
			if (!pin.p) { grayVec.resize(px); gray = grayVec.data(); } // no page-locked memory to be had: the library stages the copy
			else memcpy(bgrUp, bgr.data(), px * 3);
			for (size_t k = 0; k < px; ++k) // Types.inl:2354-2400 toGray, normalised
				gray[k] = (0.114f * bgr[3 * k] + 0.587f * bgr[3 * k + 1] + 0.299f * bgr[3 * k + 2]) / 255.f;
			for (size_t d = 0; d < devs.size(); ++d) {
				const bool g = needGray[d][(size_t)t] != 0;
				if (!g && d != 0) continue; // this device never touches the image
				std::lock_guard<std::mutex> lk(devs[d].upMu); // one HIP stream per context: uploads one after the other, while the other cores decode
				if (hcmvs_upload_view(devs[d].ctx, im.id, im.w, im.h, g ? gray : nullptr, bgrUp, im.cam.K, im.cam.R, im.cam.C) != HCMVS_OK) {
					std::lock_guard<std::mutex> e(errMu);
					if (loadError.empty()) loadError = std::string("upload of image '") + paths[t] + "' failed: " + hcmvs_last_error(devs[d].ctx);
				}
			}
		}
	};
	createThread.join();
	for (auto& d : devs)
		if (d.createRc != HCMVS_OK) { fprintf(stderr, "error: device %d is not a usable MI355X (there is no CPU path)\n", d.ordinal); return EXIT_FAILURE; }
	hcmvs_ctx* ctx = devs[0].ctx; // the context of the post-filters and the fusion
	if (hipSetDevice(o.device) != hipSuccess) { fprintf(stderr, "error: hipSetDevice failed\n"); return EXIT_FAILURE; }
	if (nDev > 1 && o.viewspread) { fprintf(stderr, "error: --n-viewspread 1 runs on one device: every estimate reads the depth maps of its source views, which other devices would hold (drop --devices)\n"); return EXIT_FAILURE; }
	if (nDev > 1 && o.postFilterInterleave) { fprintf(stderr, "error: --n-postfilter-interleave 1 estimates one image at a time and runs on one device (drop --devices)\n"); return EXIT_FAILURE; }
	std::vector<uint32_t> todo;
	for (auto& im : images) {
		if (!im.valid) continue;
		if (!selected[im.id]) {
			if (o.verbosity > 1) printf("Reference image %3u has not enough images in view\n", im.id);
			continue;
		}
		todo.push_back(im.id);
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
	hcmvs_params prm;
	hcmvs_default_params(&prm);
	prm.adapthalfwin = o.adaptHalfWin; prm.n_estimation_iters = o.estimationIters; prm.n_external_iters = o.estimationItersExternal;
	prm.propagate_halfwin = o.propagateHalfWin; prm.propagate_step = o.propagateStep; prm.photometric_flow = o.photometricFlow; prm.seed = o.seed;

	// the order of the fusion and of the post-filters' fusion: best connected images first (SceneDensify.cpp:3285-3302).  It also
	// deals the reference images to the devices: position k of it goes to device k mod N, so that the devices
	// are loaded alike.  A device holds the gray image of its own reference images and of their source views only.
	std::vector<uint32_t> fuseOrder(todo);
	std::stable_sort(fuseOrder.begin(), fuseOrder.end(), [&](uint32_t a, uint32_t b) { return images[a].neighbors.size() > images[b].neighbors.size(); });
	for (size_t k = 0; k < fuseOrder.size(); ++k) images[fuseOrder[k]].dev = (int)(k % (size_t)nDev);
	if (nDev > 1) {
		for (auto& v : needGray) std::fill(v.begin(), v.end(), 0);
		for (uint32_t id : todo) {
			needGray[(size_t)images[id].dev][id] = 1;
			for (uint32_t s : images[id].srcs) needGray[(size_t)images[id].dev][s] = 1; // (srcs still holds scene image ids here)
		}
	}

	// What has to fit into a device (bytes per pixel of an image): resident per reference image of the device -- maps 20, hint maps 16
	// (restore variant), gray + colour + gradient 8; per source view the 2 x 2 footprints 16; per image of a batch the working state 24.
	// With --n-filter the first device also holds the stage's staging slabs and one image's z-buffer keys.
	// The first device also holds colour + gradient (4) and, with several devices, a copy of the maps (20) of EVERY image, the per-pass
	// tables of the fusion (12 B per pixel and neighbour of the largest image + 40 B per pixel) and the device copy of the cloud
	// (about half a point per pixel: 31 B, + 8 B per view entry).  The batch shrinks until the first device fits; a scene that does
	// not fit at one image per launch is refused here, before anything is uploaded (DESIGN.md section 4 has configs[3] in numbers).
	{
		size_t maxPx = 0, allPx = 0;
		for (uint32_t id : todo) { const size_t px = (size_t)images[id].w * images[id].h; maxPx = std::max(maxPx, px); allPx += px; }
		for (int d = 0; d < nDev; ++d) {
			size_t freeB = 0, totalB = 0;
			HIPOK(hipSetDevice(devs[(size_t)d].ordinal));
			HIPOK(hipMemGetInfo(&freeB, &totalB));
			size_t ownPx = 0, grayPx = 0;
			for (uint32_t id : todo) if (images[id].dev == d) ownPx += (size_t)images[id].w * images[id].h;
			for (size_t i = 0; i < images.size(); ++i) if (images[i].valid && needGray[(size_t)d][i]) grayPx += (size_t)images[i].w * images[i].h;
			size_t resident = ownPx * (size_t)(20 + (o.restoreHypothesis ? 16 : 0)) + grayPx * (size_t)(8 + 16) + ((size_t)1 << 30);
			if (d == 0) {
				size_t maxNb = 1;
				for (uint32_t id : todo) maxNb = std::max(maxNb, std::min<size_t>(images[id].neighbors.size(), 31));
				resident += allPx * 4 + (nDev > 1 ? allPx * 20 : 0) + maxPx * (12 * maxNb + 40);
				// --n-filter: the staging of the filtered maps (8 B per pixel of the scene) and the z-buffer keys of a batch of one image with 8
				// neighbours (the stage takes more images per batch when more memory is free)
				if (o.nFilter) resident += allPx * 8 + maxPx * 8 * 8;
				// the cloud: counted first when large (see the fusion below), so what is reserved is what it holds -- taken here as 0.2
				// points per pixel (the reference reserves 0.15, SceneDensify.cpp:3298) with 3 view entries each
				if (o.fusionMode != 1) resident += (allPx * 39 > ((size_t)4 << 30) && o.fuseCount != 0) ? allPx / 5 * (31 + 3 * 8) : allPx / 2 * 31 + allPx * 8;
			}
			int batch = o.batch;
			while (batch > 1 && resident + (size_t)batch * maxPx * 24 > freeB) batch /= 2;
			if (resident + (size_t)batch * maxPx * 24 > freeB) {
				fprintf(stderr, "error: the scene does not fit device %d: %.1f GiB needed for its share (%zu of %zu images; maps, images, source footprints%s), "
				                "%.1f GiB free.  Use more devices (--devices), a coarser --resolution-level or fewer --number-views\n",
				        devs[(size_t)d].ordinal, (resident + (size_t)batch * maxPx * 24) / 1073741824.0, (size_t)std::count_if(todo.begin(), todo.end(), [&](uint32_t id) { return images[id].dev == d; }),
				        todo.size(), d == 0 ? ", the whole scene's maps, fusion tables and cloud" : "", freeB / 1073741824.0);
				return EXIT_FAILURE;
			}
			o.batch = std::min(o.batch, batch);
			if (o.verbosity > 2) printf("Device %d (context %d of %d): %.1f GiB resident + %.1f GiB per batch of %d, %.1f GiB free\n", devs[(size_t)d].ordinal, d, nDev,
			                            resident / 1073741824.0, (size_t)batch * maxPx * 24 / 1073741824.0, batch, freeB / 1073741824.0);
		}
		HIPOK(hipSetDevice(o.device));
	}

	// skip-if-exists resume (SceneDensify.cpp:3865-3880: "try to load already compute depth-map for this image"): an image whose
	// final depth map of this size is in the working folder is loaded instead of estimated
	std::vector<char> resumed(images.size(), 0);
	std::vector<uint32_t> work; // the images to estimate, in todo order
	for (uint32_t id : todo) {
		DmapFile hdr;
		if (o.resume && load_dmap(map_path(o.workdir, "/depth%04u.dmap", id), hdr, 7, true) && hdr.w == images[id].w && hdr.h == images[id].h) resumed[id] = 1;
		else { work.push_back(id); devs[(size_t)images[id].dev].work.push_back(id); }
	}
	for (uint32_t id : todo) {
		if (!resumed[id]) continue;
		ImageData& im = images[id];
		DmapFile m;
		if (!load_dmap(map_path(o.workdir, "/depth%04u.dmap", id), m, 7)) { fprintf(stderr, "error: invalid depth-map '%s'\n", map_path(o.workdir, "/depth%04u.dmap", id).c_str()); return EXIT_FAILURE; }
		const size_t n = (size_t)im.w * im.h;
		im.dMin = m.dMin; im.dMax = m.dMax;
		HIPOK(hipSetDevice(devs[(size_t)im.dev].ordinal));
		HIPOK(hipMalloc(&im.dDepth, n * 4)); HIPOK(hipMalloc(&im.dNormal, n * 12)); HIPOK(hipMalloc(&im.dConf, n * 4));
		HIPOK(hipMemcpy(im.dDepth, m.d.data(), n * 4, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(im.dNormal, m.n.data(), n * 12, hipMemcpyHostToDevice));
		HIPOK(hipMemcpy(im.dConf, m.c.data(), n * 4, hipMemcpyHostToDevice));
		if (o.verbosity > 1) printf("Depth-map for image %3u loaded from '%s' (not estimated again)\n", id, map_path(o.workdir, "/depth%04u.dmap", id).c_str());
	}
	HIPOK(hipSetDevice(o.device));

	// batches: images of one device and one lane layout class (up to 8 source views, or 9..16) share a launch.  The loader serves the
	// devices in turn (first batch of every device first).
	struct Batch { int dev; std::vector<uint32_t> ids; };
	std::vector<Batch> batches;
	{
		std::vector<std::vector<Batch>> perDev((size_t)nDev);
		for (int d = 0; d < nDev; ++d) {
			std::map<int, std::vector<uint32_t>> byClass;
			for (uint32_t id : devs[(size_t)d].work) byClass[images[id].srcs.size() <= 8 ? 8 : 16].push_back(id);
			for (auto& g : byClass)
				for (size_t b0 = 0; b0 < g.second.size(); b0 += (size_t)o.batch)
					perDev[(size_t)d].push_back(Batch{d, std::vector<uint32_t>(g.second.begin() + (long)b0, g.second.begin() + (long)std::min(g.second.size(), b0 + (size_t)o.batch))});
		}
		for (size_t k = 0;; ++k) {
			bool any = false;
			for (int d = 0; d < nDev; ++d) if (k < perDev[(size_t)d].size()) { batches.push_back(perDev[(size_t)d][k]); any = true; }
			if (!any) break;
		}
	}

	// ---- the loader: initial maps of batch k + 1 while batch k is estimated (outer iteration 0) ----
	//   nMinViewsTrustPoint < 2      splat of the sparse points (SceneDensify.cpp:783-808)
	//   initTriangulate != 0         Delaunay triangulation of the sparse points (DepthMapsData::InitDepthMap, DepthMap.cpp:1796-1936)
	//   initTriangulate == 0         the previous run's maps, <working-folder>/depthmap/depth%04u.dmap + normalmap/normal%04u.dmap
	//                                (what run.sh moves between the stages; SceneDensify.cpp:527-553), else <working-folder>/depth%04u.dmap
	// restore-hypothesis: the previous level's maps, enlarged with INTER_AREA, are the extra last-sweep hypothesis and widen the
	// depth range (restore/libs/MVS/SceneDensify.cpp:508-532)
	std::vector<Prepared> prepared(batches.size());
	std::mutex prepMu; std::condition_variable prepCv;
	std::string prepError;
	auto previous_maps = [&](uint32_t id, DmapFile& out) -> bool {
		DmapFile dm, nm;
		if (load_dmap(map_path(o.workdir, "/depthmap/depth%04u.dmap", id), dm, 1) && load_dmap(map_path(o.workdir, "/normalmap/normal%04u.dmap", id), nm, 2) &&
		    dm.w == nm.w && dm.h == nm.h) {
			out.w = dm.w; out.h = dm.h; out.d.swap(dm.d); out.n.swap(nm.n);
			return true;
		}
		return load_dmap(map_path(o.workdir, "/depth%04u.dmap", id), out, 3);
	};
	auto loader = [&]() {
		// page-locked staging, one copy stream per device: a pageable hipMemcpy of the initial maps (33 MB per 1080p image) crawls
		std::vector<std::unique_ptr<Uploader>> ups((size_t)nDev);
		for (int d = 0; d < nDev; ++d) {
			ups[(size_t)d].reset(new Uploader);
			if (hipSetDevice(devs[(size_t)d].ordinal) != hipSuccess || !ups[(size_t)d]->init()) { std::lock_guard<std::mutex> g(prepMu); prepError = "no copy stream for the loader"; prepCv.notify_all(); return; }
		}
		for (size_t b = 0; b < batches.size(); ++b) {
			const std::vector<uint32_t>& ids = batches[b].ids;
			Uploader& up = *ups[(size_t)batches[b].dev];
			if (hipSetDevice(devs[(size_t)batches[b].dev].ordinal) != hipSuccess) { std::lock_guard<std::mutex> g(prepMu); prepError = "hipSetDevice failed in the loader"; prepCv.notify_all(); return; }
			std::vector<InitMaps> maps(ids.size());
#pragma omp parallel for schedule(dynamic, 1)
			for (long k = 0; k < (long)ids.size(); ++k) {
				ImageData& im = images[ids[k]];
				InitMaps& M = maps[k];
				const size_t n = (size_t)im.w * im.h;
				std::vector<float> pts;
				for (uint32_t idx : im.points) { pts.push_back(verts[idx].X[0]); pts.push_back(verts[idx].X[1]); pts.push_back(verts[idx].X[2]); }
				M.d.assign(n, 0.f); M.n.assign(3 * n, 0.f);
				if (o.minViewsTrustPoint < 2) {
					// the context-free form: the loader's workers never touch the context (it is not thread-safe, and the main thread is
					// registering views meanwhile)
					if (hcmvs_splat_points(im.w, im.h, im.cam.K, im.cam.R, im.cam.C, pts.data(), (int32_t)im.points.size(), M.d.data(), M.n.data(), &im.dMin, &im.dMax) != HCMVS_OK) M.failed = 1;
				} else if (o.initTriangulate || o.restoreHypothesis) { // the `restore` binary always triangulates (restore/libs/MVS/SceneDensify.cpp:508-511)
					if (hcmvs_triangulate_points(im.w, im.h, im.cam.K, im.cam.R, im.cam.C, pts.data(), (int32_t)im.points.size(), 0.f, 1, M.d.data(), M.n.data(),
					                             &im.dMin, &im.dMax) != HCMVS_OK) M.failed = 1;
				} else {
					DmapFile pm;
					if (!previous_maps(im.id, pm)) { M.failed = 2; continue; }
					if (o.verbosity > 2) printf("read  :  %s (%dx%d -> %dx%d)\n", map_path(o.workdir, "/depthmap/depth%04u.dmap", im.id).c_str(), pm.w, pm.h, im.w, im.h);
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
					if (!(hi > 0.f)) { M.failed = 3; continue; }
					im.dMin = lo * 0.9f; im.dMax = hi * 1.1f;
				}
				if (o.restoreHypothesis && !M.failed) {
					DmapFile pm;
					if (!previous_maps(im.id, pm) || pm.w > im.w || pm.h > im.h) { M.failed = 2; continue; }
					M.hd.resize(n); M.hn.resize(3 * n);
					// cv::resize(..., INTER_AREA) to the current size (restore/libs/MVS/SceneDensify.cpp:523-524)
					if (hcmvs_resize_area_up(pm.d.data(), pm.w, pm.h, 1, M.hd.data(), im.w, im.h) != HCMVS_OK ||
					    hcmvs_resize_area_up(pm.n.data(), pm.w, pm.h, 3, M.hn.data(), im.w, im.h) != HCMVS_OK) { M.failed = 2; continue; }
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
			}
			Prepared res;
			for (size_t k = 0; k < ids.size() && !res.failed; ++k) if (maps[k].failed) { res.failed = maps[k].failed; res.failedId = ids[k]; }
			for (size_t k = 0; k < ids.size() && !res.failed; ++k) {
				ImageData& im = images[ids[k]];
				const size_t n = (size_t)im.w * im.h;
				bool ok = hipMalloc(&im.dDepth, n * 4) == hipSuccess && hipMalloc(&im.dNormal, n * 12) == hipSuccess && hipMalloc(&im.dConf, n * 4) == hipSuccess &&
				          up.copy(im.dDepth, maps[k].d.data(), n * 4) && up.copy(im.dNormal, maps[k].n.data(), n * 12) && hipMemsetAsync(im.dConf, 0, n * 4, up.s) == hipSuccess;
				if (ok && o.restoreHypothesis)
					ok = hipMalloc(&im.dHintDepth, n * 4) == hipSuccess && hipMalloc(&im.dHintNormal, n * 12) == hipSuccess &&
					     up.copy(im.dHintDepth, maps[k].hd.data(), n * 4) && up.copy(im.dHintNormal, maps[k].hn.data(), n * 12);
				if (!ok) { res.failed = 4; res.failedId = ids[k]; }
			}
			if (!res.failed && !up.drain()) { res.failed = 4; res.failedId = ids.empty() ? 0 : ids[0]; }
			res.ready = true;
			{
				std::lock_guard<std::mutex> g(prepMu);
				prepared[b] = res;
			}
			prepCv.notify_all();
			if (res.failed) return;
		}
	};
	std::thread loaderThread(loader);
	struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } loaderJoin{loaderThread};
	const double tDecode = now_s();
	load_images();
	if (o.verbosity > 2) printf("Start-up: %.2f s until the images are decoded (scene file, headers, view selection, device context), %.2f s decoding + uploading them\n", tDecode - tStart, now_s() - tDecode);
	if (!loadError.empty()) { fprintf(stderr, "error: %s\n", loadError.c_str()); return EXIT_FAILURE; }
	if (o.verbosity > 1) printf("Scene loaded: %zu images (%u calibrated), %zu sparse points\n", images.size(), nValid, verts.size());
	const double tLoaded = now_s();
	// neighbours whose footprint scale differs by >= 15 % are resampled on the device and registered as views of their own
	// (DepthData::ViewData::ScaleImage + Image::GetCamera, SceneDensify.cpp:372-374); one copy per (image, new size) and device
	{
		std::map<std::pair<uint32_t, std::pair<int, int>>, uint32_t> scaled;
		std::vector<std::map<uint32_t, bool>> made((size_t)nDev);
		uint32_t nextId = 0x8000;
		for (uint32_t id : todo) {
			ImageData& im = images[id];
			im.srcImages = im.srcs;
			for (size_t k = 0; k < im.srcs.size(); ++k) {
				if (im.srcScale[k] == 1.f) continue;
				const ImageData& sv = images[im.srcs[k]];
				const std::pair<int, int> size((int)std::lrint((double)sv.w * im.srcScale[k]), (int)std::lrint((double)sv.h * im.srcScale[k]));
				const auto key = std::make_pair(sv.id, size);
				auto it = scaled.find(key);
				if (it == scaled.end()) {
					if (nextId >= 65536) { fprintf(stderr, "error: too many resampled neighbour views\n"); return EXIT_FAILURE; }
					it = scaled.emplace(key, nextId++).first;
				}
				if (!made[(size_t)im.dev].count(it->second)) {
					hcmvs_ctx* dctx = devs[(size_t)im.dev].ctx;
					if (hcmvs_rescale_view(dctx, sv.id, it->second, im.srcScale[k]) != HCMVS_OK) { fprintf(stderr, "error: resampling image %u failed (%s)\n", sv.id, hcmvs_last_error(dctx)); return EXIT_FAILURE; }
					if (o.verbosity > 2) printf("Image %3u resampled by %.2f to %dx%d as view %u\n", sv.id, im.srcScale[k], size.first, size.second, it->second);
					made[(size_t)im.dev][it->second] = true;
				}
				im.srcs[k] = it->second;
			}
		}
		HIPOK(hipSetDevice(o.device));
	}
	// --ignore-mask-label (DepthEstimator::ImportIgnoreMask, DepthMap.cpp:319-348): the labels split at every ',' (empty tokens kept,
	// Util::strSplit) and read with atoi; every image to estimate gets the keep-mask of its label image on the context that estimates it
	if (!o.ignoreMaskLabel.empty()) {
		std::vector<int32_t> labels;
		for (size_t b = 0;;) {
			const size_t e = o.ignoreMaskLabel.find(',', b);
			labels.push_back((int32_t)atoi(o.ignoreMaskLabel.substr(b, e == std::string::npos ? std::string::npos : e - b).c_str()));
			if (e == std::string::npos) break;
			b = e + 1;
		}
		size_t nMasked = 0, pxAll = 0, pxIgnored = 0;
		for (uint32_t id : todo) {
			const ImageData& im = images[id];
			// the fork's rule (Scene.cpp:119-126): getFilePath(name) + "/seman/" + getFileName(name) + ".quad.png", read here as its binary
			// Netpbm siblings.  A name without a folder resolves against the image's own folder (the fork makes it root-absolute).
			const size_t sl = im.name.find_last_of('/');
			std::string stem = sl == std::string::npos ? im.name : im.name.substr(sl + 1);
			if (stem.find_last_of('.') != std::string::npos) stem = stem.substr(0, stem.find_last_of('.'));
			const std::string base = dirname_of(paths[id]) + "/seman/" + stem + ".quad";
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
			hcmvs_ctx* dctx = devs[(size_t)im.dev].ctx;
			std::vector<uint8_t> keep((size_t)im.w * im.h);
			if (hcmvs_set_ignore_mask(dctx, id, lab.data(), lw, lh, labels.data(), (int32_t)labels.size()) != HCMVS_OK ||
			    hcmvs_get_ignore_mask(dctx, id, keep.data()) != HCMVS_OK) {
				fprintf(stderr, "error: the ignore mask of image %u failed (%s)\n", id, hcmvs_last_error(dctx));
				return EXIT_FAILURE;
			}
			++nMasked; pxAll += keep.size();
			pxIgnored += (size_t)std::count(keep.begin(), keep.end(), (uint8_t)0);
		}
		HIPOK(hipSetDevice(o.device));
		if (o.verbosity > 1)
			printf("Ignore mask (labels %s): %zu of %zu images masked, %.2f %% of their pixels ignored\n", o.ignoreMaskLabel.c_str(), nMasked, todo.size(),
			       pxAll ? 100.0 * (double)pxIgnored / (double)pxAll : 0.0);
	}

	// ---- the saver: copies + files of the final maps, behind the estimation ----
	Saver sv;
	auto save_files = [&](const SaveJob& j) -> bool {
		const ImageData& im = images[j.id];
		// depth%04u.dmap: the complete DepthData (what the fusion stage of the reference loads, SceneDensify.cpp:3292); depthmap/ +
		// normalmap/: the hand-off pair the next stage of run.sh picks up (DepthMap.h:76-80, SceneDensify.cpp:3984-3988; raw 'DR'
		// content instead of the reference's boost archive)
		return save_dmap(map_path(o.workdir, "/depth%04u.dmap", j.id), im, j.d.data(), j.n.data(), j.c.data()) &&
		       save_dmap(map_path(o.workdir, "/depthmap/depth%04u.dmap", j.id), im, j.d.data(), nullptr, nullptr) &&
		       save_dmap(map_path(o.workdir, "/normalmap/normal%04u.dmap", j.id), im, nullptr, j.n.data(), nullptr);
	};
	auto copier = [&]() {
		std::vector<hipStream_t> css((size_t)nDev, nullptr); // a map is copied on a stream of the device that holds it
		for (int d = 0; d < nDev; ++d)
			if (hipSetDevice(devs[(size_t)d].ordinal) != hipSuccess || hipStreamCreateWithFlags(&css[(size_t)d], hipStreamNonBlocking) != hipSuccess) {
				std::lock_guard<std::mutex> g(sv.mu); sv.error = "no copy stream"; sv.cv.notify_all(); return;
			}
		for (;;) {
			uint32_t id;
			{
				std::unique_lock<std::mutex> g(sv.mu);
				sv.cv.wait(g, [&] { return !sv.toCopy.empty() || sv.closing || !sv.error.empty(); });
				if (!sv.error.empty() || (sv.toCopy.empty() && sv.closing)) break;
				id = sv.toCopy.front(); sv.toCopy.pop_front();
				const size_t need = (size_t)images[id].w * images[id].h * 20;
				sv.cv.wait(g, [&] { return sv.bytesQueued + need <= Saver::kMaxQueuedBytes || sv.toWrite.empty() || !sv.error.empty(); });
				if (!sv.error.empty()) break;
				sv.bytesQueued += need;
			}
			const ImageData& im = images[id];
			const size_t n = (size_t)im.w * im.h;
			std::unique_ptr<SaveJob> j(new SaveJob);
			j->id = id; j->d.resize(n); j->n.resize(3 * n); j->c.resize(n);
			hipStream_t cs = css[(size_t)im.dev];
			const bool ok = hipSetDevice(devs[(size_t)im.dev].ordinal) == hipSuccess &&
			                hipMemcpyAsync(j->d.data(), im.dDepth, n * 4, hipMemcpyDeviceToHost, cs) == hipSuccess &&
			                hipMemcpyAsync(j->n.data(), im.dNormal, n * 12, hipMemcpyDeviceToHost, cs) == hipSuccess &&
			                hipMemcpyAsync(j->c.data(), im.dConf, n * 4, hipMemcpyDeviceToHost, cs) == hipSuccess && hipStreamSynchronize(cs) == hipSuccess;
			std::lock_guard<std::mutex> g(sv.mu);
			if (!ok) sv.error = "copy of a depth map to the host failed";
			else { sv.toWrite.push_back(std::move(j)); ++sv.copied; }
			sv.cv.notify_all();
		}
		for (int d = 0; d < nDev; ++d) if (css[(size_t)d]) { (void)hipSetDevice(devs[(size_t)d].ordinal); (void)hipStreamDestroy(css[(size_t)d]); }
	};
	auto writer = [&]() {
		for (;;) {
			std::unique_ptr<SaveJob> j;
			{
				std::unique_lock<std::mutex> g(sv.mu);
				sv.cv.wait(g, [&] { return !sv.toWrite.empty() || (sv.closing && sv.copied == sv.submitted) || !sv.error.empty(); });
				if (sv.toWrite.empty()) break;
				j = std::move(sv.toWrite.front()); sv.toWrite.pop_front();
			}
			const bool ok = save_files(*j);
			std::lock_guard<std::mutex> g(sv.mu);
			sv.bytesQueued -= (size_t)images[j->id].w * images[j->id].h * 20;
			++sv.written;
			if (!ok && sv.error.empty()) sv.error = "can not write '" + map_path(o.workdir, "/depth%04u.dmap", j->id) + "'";
			sv.cv.notify_all();
		}
	};
	(void)mkdir((o.workdir + "/depthmap").c_str(), 0777);
	(void)mkdir((o.workdir + "/normalmap").c_str(), 0777);
	std::thread copierThread(copier);
	std::vector<std::thread> writerThreads;
	for (int k = 0; k < 4; ++k) writerThreads.emplace_back(writer);
	auto saver_submit = [&](const std::vector<uint32_t>& ids) {
		std::lock_guard<std::mutex> g(sv.mu);
		for (uint32_t id : ids) { sv.toCopy.push_back(id); ++sv.submitted; }
		sv.cv.notify_all();
	};
	auto saver_close = [&]() { { std::lock_guard<std::mutex> g(sv.mu); sv.closing = true; } sv.cv.notify_all(); };
	struct SaverJoin { std::thread& c; std::vector<std::thread>& w; Saver& s; ~SaverJoin() { { std::lock_guard<std::mutex> g(s.mu); s.closing = true; if (s.error.empty() && s.copied != s.submitted) s.error = "aborted"; } s.cv.notify_all(); if (c.joinable()) c.join(); for (auto& t : w) if (t.joinable()) t.join(); } } saverJoin{copierThread, writerThreads, sv};

	const double tInit = now_s();
	double tPostfilter = 0;
	const bool filterOnLast = (o.postFilter && (o.estimationItersExternal - 1 == 1 || o.estimationItersExternal - 1 == 2)) ||
	                          (o.postFilterInterleave && o.viewspread && o.estimationItersExternal - 1 >= 1); // (the main thread hands the last iteration's maps to the saver)
	// one launch set for the reference images `ids` (all of device context d)
	auto estimate_images = [&](int d, const std::vector<uint32_t>& ids, const hcmvs_params& pr, std::string& err) -> bool {
		hcmvs_ctx* dctx = devs[(size_t)d].ctx;
		std::vector<hcmvs_batch_item> items;
		for (uint32_t id : ids) {
			ImageData& im = images[id];
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
		if (o.verbosity > 2)
			for (const auto& itx : items)
				printf("Depth-map for image %3u estimated using %2d images: %dx%d (outer iteration %d, batch %.0f ms%s)\n", itx.ref_id,
				       itx.n_src, images[itx.ref_id].w, images[itx.ref_id].h, pr.it_external, st.ms_total, nDev > 1 ? (", device context " + std::to_string(d)).c_str() : "");
		return true;
	};
	// The first device filters and fuses the whole scene: it holds a copy (g*) of the maps the other devices estimate.  gather: owner ->
	// first device, scatter: back (after the post-filters changed them).  Peer copies over xGMI (hipMemcpyPeerAsync); two contexts on one
	// GPU (--devices 0,0) copy device to device.  Single process: nothing is replicated, nobody else filters.
	hipStream_t xs = nullptr;
	HIPOK(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking));
	struct StreamGuard { hipStream_t s; ~StreamGuard() { if (s) (void)hipStreamDestroy(s); } } xsGuard{xs};
	auto exchange_maps = [&](bool toFirst) -> bool {
		const int ord0 = devs[0].ordinal;
		if (hipSetDevice(ord0) != hipSuccess) return false; // the copies on the first device are allocated there
		for (uint32_t id : todo) {
			ImageData& im = images[id];
			const size_t n = (size_t)im.w * im.h;
			if (im.dev == 0) { im.gDepth = im.dDepth; im.gNormal = im.dNormal; im.gConf = im.dConf; continue; }
			if (!im.gDepth && (hipMalloc(&im.gDepth, n * 4) != hipSuccess || hipMalloc(&im.gNormal, n * 12) != hipSuccess || hipMalloc(&im.gConf, n * 4) != hipSuccess)) return false;
			const int ord = devs[(size_t)im.dev].ordinal;
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
	};
	// the maps and neighbour lists the post-filters' fusion works on: every image of the scene, on the first device
	const std::vector<uint32_t>& filterOrder = fuseOrder;
	auto register_maps = [&]() -> bool {
		for (uint32_t id : todo) {
			ImageData& im = images[id];
			std::vector<uint32_t> nb;
			for (const auto& x : im.neighbors) if (std::find(todo.begin(), todo.end(), x.id) != todo.end()) nb.push_back(x.id);
			if (nb.size() > 31) nb.resize(31);
			if (hcmvs_set_depthmap_device(ctx, id, im.gDepth ? im.gDepth : im.dDepth, im.gNormal ? im.gNormal : im.dNormal, im.gConf ? im.gConf : im.dConf, im.dMin, im.dMax) != HCMVS_OK ||
			    hcmvs_set_neighbors(ctx, id, nb.data(), (int32_t)nb.size()) != HCMVS_OK) {
				fprintf(stderr, "error: registering the maps of image %u failed (%s)\n", id, hcmvs_last_error(ctx));
				return false;
			}
		}
		return true;
	};
	// --n-viewspread (one device): what the source views offer.  Batch schedule: before every outer iteration >= 1 the maps of all images are
	// copied into a second buffer set (20 B per pixel of the scene) -- every estimate of the iteration reads its source views as the previous
	// iteration left them, post-filters included.  Interleaved schedule: the live maps (the reference's order; an image is never its own
	// source view, and one image is estimated per call).
	struct SpreadSnap { float *d = nullptr, *n = nullptr, *c = nullptr; };
	std::map<uint32_t, SpreadSnap> spreadSnap;
	struct SnapFree { std::map<uint32_t, SpreadSnap>& m; ~SnapFree() { for (auto& kv : m) for (float* q : {kv.second.d, kv.second.n, kv.second.c}) if (q) (void)hipFree(q); } } snapFree{spreadSnap};
	auto offer_spread_maps = [&](bool live, std::string& err) -> bool {
		if (hcmvs_synchronize(ctx) != HCMVS_OK) { err = hcmvs_last_error(ctx); return false; }
		for (uint32_t id : todo) {
			ImageData& im = images[id];
			if (!im.dDepth || !im.dNormal || !im.dConf) continue;
			const size_t n = (size_t)im.w * im.h;
			const float *sd = im.dDepth, *sn = im.dNormal, *sc = im.dConf;
			if (!live) {
				SpreadSnap& sp = spreadSnap[id];
				if (!sp.d && (hipMalloc(&sp.d, n * 4) != hipSuccess || hipMalloc(&sp.n, n * 12) != hipSuccess || hipMalloc(&sp.c, n * 4) != hipSuccess)) { err = "no device memory for the view-spread copy of the depth maps (20 B per pixel of the scene)"; return false; }
				if (hipMemcpyAsync(sp.d, im.dDepth, n * 4, hipMemcpyDeviceToDevice, xs) != hipSuccess || hipMemcpyAsync(sp.n, im.dNormal, n * 12, hipMemcpyDeviceToDevice, xs) != hipSuccess ||
				    hipMemcpyAsync(sp.c, im.dConf, n * 4, hipMemcpyDeviceToDevice, xs) != hipSuccess) { err = "copying the depth maps for view spread failed"; return false; }
				sd = sp.d; sn = sp.n; sc = sp.c;
			}
			if (hcmvs_set_spread_maps_device(ctx, id, sd, sn, sc) != HCMVS_OK) { err = hcmvs_last_error(ctx); return false; }
		}
		if (hipStreamSynchronize(xs) != hipSuccess) { err = "copying the depth maps for view spread failed"; return false; }
		return true;
	};
	if (o.viewspread) CHK(hcmvs_set_viewspread(ctx, 1));
	// an outer iteration that the main thread runs image after image: the interleaved schedule, where it filters and -- with view spread -- in
	// every outer iteration >= 1
	auto serial_iteration = [&](int it) { return o.postFilterInterleave && !work.empty() && ((o.postFilter && (it == 1 || it == 2)) || (o.viewspread && it >= 1)); };
	const int nMinViewsFuse = std::min<int>(o.numberViewsFuse, (int)images.size());
	// outer iterations over all images (SceneDensify.cpp:3684).  Every device context has a host thread that estimates the context's
	// batches; where an outer iteration ends with the post-filters the threads meet, the main thread gathers the maps on the first
	// device, filters, hands the filtered maps back and lets the threads go on.
	std::mutex runMu; std::condition_variable runCv;
	std::string runError;
	int arrived = 0, released = -1; // workers waiting at the end of a filtered outer iteration; the last iteration whose filters are done
	auto wait_prepared = [&](size_t b) -> bool {
		std::unique_lock<std::mutex> g(prepMu);
		prepCv.wait(g, [&] { return prepared[b].ready || !prepError.empty(); });
		if (!prepError.empty()) { fprintf(stderr, "error: %s\n", prepError.c_str()); return false; }
		const Prepared& pr = prepared[b];
		if (pr.failed == 2) { fprintf(stderr, "error: can not read the previous level's maps of image %u ('%s/depthmap/depth%04u.dmap' + normalmap, or '%s/depth%04u.dmap')\n", pr.failedId, o.workdir.c_str(), pr.failedId, o.workdir.c_str(), pr.failedId); return false; }
		if (pr.failed == 3) { fprintf(stderr, "error: the previous level's depth map of image %u holds no valid depth\n", pr.failedId); return false; }
		if (pr.failed) { fprintf(stderr, "error: initialisation of image %u failed (%s)\n", pr.failedId, pr.failed == 4 ? "device memory" : "no sparse point in front of the image"); return false; }
		return true;
	};
	auto fail_run = [&](const std::string& msg) { { std::lock_guard<std::mutex> g(runMu); if (runError.empty()) runError = msg; } runCv.notify_all(); };
	auto worker = [&](int d) {
		if (hipSetDevice(devs[(size_t)d].ordinal) != hipSuccess) { fail_run("hipSetDevice failed in an estimation thread"); return; }
		hcmvs_params pr = prm;
		for (int it = 0; it < o.estimationItersExternal; ++it) {
			pr.it_external = it;
			const bool last = it == o.estimationItersExternal - 1;
			const bool filtered = o.postFilter && (it == 1 || it == 2) && !work.empty();
			const bool serial = serial_iteration(it);
			if (!serial) { // (the interleaved mode runs on the main thread, one device)
				if (o.viewspread && it >= 1) { // (one device: this is the only worker, and the previous iteration's filters are done)
					std::string err;
					if (!offer_spread_maps(false, err)) { fail_run(err); return; }
				}
				for (size_t b = 0; b < batches.size(); ++b) {
					if (batches[b].dev != d) continue;
					{ std::lock_guard<std::mutex> g(runMu); if (!runError.empty()) return; }
					if (it == 0 && !wait_prepared(b)) { fail_run("initialisation failed"); return; }
					std::string err;
					if (!estimate_images(d, batches[b].ids, pr, err)) { fail_run(err); return; }
					if (last && !filterOnLast && !o.nFilter) saver_submit(batches[b].ids); // final maps of this batch: off to the host while the next batch runs
				}
			}
			if (filtered || serial) { // meet the others; the main thread filters
				std::unique_lock<std::mutex> g(runMu);
				++arrived;
				runCv.notify_all();
				runCv.wait(g, [&] { return released >= it || !runError.empty(); });
				if (!runError.empty()) return;
			}
		}
	};
	std::vector<std::thread> workers;
	for (int d = 0; d < nDev; ++d) workers.emplace_back(worker, d);
	struct WorkersJoin { std::vector<std::thread>& w; std::mutex& mu; std::condition_variable& cv; std::string& err;
		~WorkersJoin() { { std::lock_guard<std::mutex> g(mu); if (err.empty()) err = "aborted"; } cv.notify_all(); for (auto& t : w) if (t.joinable()) t.join(); } } workersJoin{workers, runMu, runCv, runError};
	for (int it = 0; it < o.estimationItersExternal; ++it) {
		const bool last = it == o.estimationItersExternal - 1;
		// SceneDensify.cpp:3916, 3939-3958: with --n-nOptimize's REMOVE_SPECKLES | FILL_GAPS bits, after the estimates of outer
		// iterations 1 and 2 every image goes through RemoveSmallSegments (in the fork: a whole fusion pass over the current maps of all
		// images) and GapInterpolation
		const bool filtered = o.postFilter && (it == 1 || it == 2) && !work.empty();
		const bool serial = serial_iteration(it);
		if (!filtered && !serial) continue;
		{ // every device has finished the estimates of this outer iteration (or, interleaved mode, is waiting for the main thread to run it)
			std::unique_lock<std::mutex> g(runMu);
			runCv.wait(g, [&] { return arrived == nDev || !runError.empty(); });
			if (!runError.empty()) { fprintf(stderr, "error: %s\n", runError.c_str()); return EXIT_FAILURE; }
			arrived = 0;
		}
		const double tp = now_s();
		if (!exchange_maps(true)) { fprintf(stderr, "error: gathering the depth maps on device %d failed\n", devs[0].ordinal); return EXIT_FAILURE; }
		if (!register_maps()) return EXIT_FAILURE;
		uint64_t filledAll = 0;
		if (serial) {
			if (o.viewspread && it >= 1) {
				std::string err;
				if (!offer_spread_maps(true, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return EXIT_FAILURE; }
			}
			// the reference's order, exactly (single-thread event loop, SceneDensify.cpp:3889-3965: EVTEstimateDepthMap(k) queues
			// EVTOptimizeDepthMap(k) FIRST): image k is filtered right after its own estimate, so its fusion sees the images > k as the
			// previous outer iteration left them and zeroes depths in them before they are estimated again.  One image per launch: the
			// exact mode, not the fast one
			hcmvs_params pr = prm;
			pr.it_external = it;
			double tf = 0;
			for (uint32_t id : work) {
				std::string err;
				if (!estimate_images(0, std::vector<uint32_t>(1, id), pr, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return EXIT_FAILURE; }
				if (!filtered) continue; // (view spread alone: image after image, nothing to filter in this outer iteration)
				const double t0 = now_s();
				uint64_t filled = 0;
				CHK(hcmvs_postfilter(ctx, id, filterOrder.data(), (int32_t)filterOrder.size(), nMinViewsFuse, 0.01f, 25.f, 7, &filled));
				filledAll += filled;
				tf += now_s() - t0;
			}
			tPostfilter += tf;
			if (o.verbosity > 1 && !filtered) printf("Depth-maps estimated image after image in outer iteration %d (the reference's order, view spread on the live maps) (%.2f s)\n", it, now_s() - tp);
			else if (o.verbosity > 1) printf("Depth-maps estimated and filtered image after image in outer iteration %d (the reference's order): %llu pixels filled "
			                            "(%.2f s, %.2f s of it post-filters)\n", it, (unsigned long long)filledAll, now_s() - tp, tf);
		} else {
			// the batch schedule of the post-filters: every image of the outer iteration has been estimated, now
			// they are filtered one image after the other (hcmvs_postfilter_sequence keeps the whole chain on the device)
			CHK(hcmvs_postfilter_sequence(ctx, work.data(), (int32_t)work.size(), filterOrder.data(), (int32_t)filterOrder.size(), nMinViewsFuse, 0.01f, 25.f, 7, &filledAll));
			tPostfilter += now_s() - tp;
			if (o.verbosity > 1) printf("Depth-maps filtered after outer iteration %d: fuse-consistency mask + gap interpolation, %llu pixels filled (%.2f s)\n", it,
			                            (unsigned long long)filledAll, now_s() - tp);
		}
		if (!exchange_maps(false)) { fprintf(stderr, "error: handing the filtered depth maps back to their devices failed\n"); return EXIT_FAILURE; }
		if (last && !o.nFilter) saver_submit(work); // (--n-filter: the files are written after the filter stage)
		{ std::lock_guard<std::mutex> g(runMu); released = it; }
		runCv.notify_all();
	}
	for (auto& t : workers) t.join();
	{
		std::lock_guard<std::mutex> g(runMu);
		if (!runError.empty()) { fprintf(stderr, "error: %s\n", runError.c_str()); return EXIT_FAILURE; }
	}
	loaderThread.join();
	double pixels = 0;
	for (uint32_t id : work) pixels += (double)images[id].w * images[id].h;
	for (auto& d : devs) if (hcmvs_synchronize(d.ctx) != HCMVS_OK) { fprintf(stderr, "error: %s\n", hcmvs_last_error(d.ctx)); return EXIT_FAILURE; }
	const double tEstimated = now_s();
	if (o.verbosity > 1)
		printf("Depth-maps estimated: %zu images (%zu resumed), %d outer x %d inner sweeps in %.2f s (%.2f Mpix/s per outer iteration; post-filters %.2f s of it); "
		       "loading + view selection %.2f s, set-up %.2f s\n",
		       work.size(), todo.size() - work.size(), o.estimationItersExternal, o.estimationIters, tEstimated - tInit,
		       pixels * o.estimationItersExternal / std::max(1e-9, tEstimated - tInit - tPostfilter) / 1e6, tPostfilter, tLoaded - tStart, tInit - tLoaded);
	// --n-filter: the filter stage (Scene::DenseReconstructionFilter, SceneDensify.cpp:4100-4185 -- the block the fork switched off at :3721-3756):
	// every image that has maps, the ones loaded through skip-if-exists included, against the first 8 of its neighbours that have maps
	// (:4116-4131), all from the maps as the estimates left them; then the filtered maps are saved (:4173) and the fusion works on them.
	// On the first device, after the gather that also precedes the fusion.
	if (o.nFilter && !todo.empty()) {
		const double tf = now_s();
		if (!exchange_maps(true)) { fprintf(stderr, "error: gathering the depth maps on device %d failed\n", devs[0].ordinal); return EXIT_FAILURE; }
		if (!register_maps()) return EXIT_FAILURE;
		// nMinViewsFilter 2, nMinViewsFilterAdjust 1, clamped to the calibrated images - 1 (SceneDensify.cpp:3014-3015)
		const int nMinViewsFilter = std::min<int>(2, (int)nValid - 1), nMinViewsFilterAdjust = std::min<int>(1, (int)nValid - 1);
		hcmvs_filter_stats fs;
		memset(&fs, 0, sizeof fs);
		CHK(hcmvs_filter_sequence(ctx, todo.data(), (int32_t)todo.size(), 8, o.nFilter == 1 ? 1 : 0, nMinViewsFilter, nMinViewsFilterAdjust, 0.01f, &fs));
		if (!exchange_maps(false)) { fprintf(stderr, "error: handing the filtered depth maps back to their devices failed\n"); return EXIT_FAILURE; }
		saver_submit(todo);
		if (o.verbosity > 1)
			printf("Depth-maps filtered: %u images, %llu/%llu depths discarded (%u skipped) in %.2f s (%s; %.2f ms on the device, batches of up to %u images)\n", fs.n_filtered,
			       (unsigned long long)fs.n_discarded, (unsigned long long)fs.n_processed, fs.n_skipped, now_s() - tf, o.nFilter == 1 ? "adjust" : "strict", fs.ms_device, fs.batch);
	}
	// the fusion mutates the depth maps: every final map must be on the host first (the files may still be on their way)
	saver_close();
	{
		std::unique_lock<std::mutex> g(sv.mu);
		sv.cv.wait(g, [&] { return sv.copied == sv.submitted || !sv.error.empty(); });
		if (!sv.error.empty()) { fprintf(stderr, "error: %s\n", sv.error.c_str()); return EXIT_FAILURE; }
	}
	const double tCopied = now_s();
	auto release_all = [&]() {
		for (auto& im : images) {
			(void)hipSetDevice(devs[(size_t)im.dev].ordinal);
			for (float* q : {im.dDepth, im.dNormal, im.dConf, im.dHintDepth, im.dHintNormal}) if (q) (void)hipFree(q);
			if (im.dev != 0) { (void)hipSetDevice(devs[0].ordinal); for (float* q : {im.gDepth, im.gNormal, im.gConf}) if (q) (void)hipFree(q); }
		}
		for (auto& d : devs) hcmvs_destroy(d.ctx);
	};
	auto wait_files = [&]() -> bool {
		std::unique_lock<std::mutex> g(sv.mu);
		sv.cv.wait(g, [&] { return sv.written == sv.submitted || !sv.error.empty(); });
		if (!sv.error.empty()) { fprintf(stderr, "error: %s\n", sv.error.c_str()); return false; }
		return true;
	};
	if (o.fusionMode == 1 || todo.empty()) {
		if (!wait_files()) return EXIT_FAILURE;
		if (o.verbosity > 1) printf("Depth-maps saved (%.2f s after the last estimate)\n", now_s() - tEstimated);
		release_all();
		return EXIT_SUCCESS;
	}
	// the maps of every image on the first device (the exchange before fusion), registered for the fusion
	if (!exchange_maps(true)) { fprintf(stderr, "error: gathering the depth maps on device %d failed\n", devs[0].ordinal); return EXIT_FAILURE; }
	if (!register_maps()) return EXIT_FAILURE;
	uint64_t capacity = 0;
	for (uint32_t id : todo) {
		const size_t n = (size_t)images[id].w * images[id].h;
		capacity += (uint64_t)(o.numberViewsFuse >= 2 ? n / 2 : n); // a fused point claims at least number-views-fuse pixels
	}
	uint64_t viewCapacity = 0;
	for (uint32_t id : todo) viewCapacity += (uint64_t)images[id].w * images[id].h; // a point merges at most one depth per image
	// The worst case (half a point per pixel, one view entry per pixel) is 39 B per pixel of the scene on the device and as much on the
	// host: 166 GB for 512 images of 3840x2160.  A large scene is therefore fused twice: a counting pass first (no cloud; a fusion
	// repeated on the maps a fusion has left makes the same decisions, so the second pass produces the cloud the first one counted),
	// then the real one with buffers of exactly the size needed.
	uint64_t countedDepths = 0;
	if ((capacity * 31 + viewCapacity * 8) > ((uint64_t)4 << 30) || o.fuseCount == 1) {
		if (o.fuseCount != 0) {
			hcmvs_cloud cnt;
			memset(&cnt, 0, sizeof cnt);
			CHK(hcmvs_set_fuse_order(ctx, o.fuseOrder));
			CHK(hcmvs_fuse_cloud(ctx, fuseOrder.data(), (int32_t)fuseOrder.size(), std::min<int>(o.numberViewsFuse, (int)images.size()), 0.01f, 25.f, o.depthweight,
			                     o.normalweight, &cnt));
			if (o.verbosity > 2) printf("Fusion counted first: %llu points, %llu view entries (worst case reserved otherwise: %llu / %llu)\n", (unsigned long long)cnt.n_points,
			                            (unsigned long long)cnt.n_view_entries, (unsigned long long)capacity, (unsigned long long)viewCapacity);
			capacity = cnt.n_points + 1; viewCapacity = cnt.n_view_entries + 1;
			countedDepths = cnt.n_depths; // the depths the fusion visited before it invalidated any (SceneDensify.cpp:3461 logs that number)
		}
	}
	// fuse: best connected images first (SceneDensify.cpp:3285-3302)
	const std::vector<uint32_t>& order = fuseOrder;
	// the complete PointCloud: points, view lists + weights (PointCloud::pointViews / pointWeights), colours, normals
	RawArray<float> xyz(capacity * 3), nrm(capacity * 3); RawArray<uint8_t> bgr(capacity * 3); RawArray<uint32_t> nviews(capacity);
	RawArray<uint32_t> viewIds(viewCapacity); RawArray<float> viewWeights(viewCapacity);
	if (capacity && (!xyz.data() || !nrm.data() || !bgr.data() || !nviews.data() || !viewIds.data() || !viewWeights.data())) {
		fprintf(stderr, "error: out of host memory for a cloud of up to %llu points\n", (unsigned long long)capacity);
		return EXIT_FAILURE;
	}
	uint64_t nPoints = 0, nDepths = 0;
	CHK(hcmvs_set_fuse_order(ctx, o.fuseOrder));
	hcmvs_cloud cl;
	memset(&cl, 0, sizeof cl);
	cl.capacity = capacity; cl.xyz = xyz.data(); cl.normal = nrm.data(); cl.bgr = bgr.data(); cl.n_views = nviews.data();
	cl.views_capacity = viewCapacity; cl.view_ids = viewIds.data(); cl.view_weights = viewWeights.data();
	CHK(hcmvs_fuse_cloud(ctx, order.data(), (int32_t)order.size(), std::min<int>(o.numberViewsFuse, (int)images.size()), 0.01f, 25.f, o.depthweight,
	                     o.normalweight, &cl));
	nPoints = cl.n_points; nDepths = countedDepths ? countedDepths : cl.n_depths;
	xyz.shrink(nPoints * 3); nrm.shrink(nPoints * 3); bgr.shrink(nPoints * 3); nviews.shrink(nPoints);
	viewIds.shrink(cl.n_view_entries); viewWeights.shrink(cl.n_view_entries);
	// --estimate-colors / --estimate-normals: 2 = estimated during fusion (above), 1 = re-estimated on the final cloud
	// (SceneDensify.cpp:3544, 3567-3572), 0 = none
	if (o.estimateColors == 1) CHK(hcmvs_estimate_point_colors(ctx, nPoints, xyz.data(), nviews.data(), viewIds.data(), bgr.data()));
	if (o.estimateNormals == 1) CHK(hcmvs_estimate_point_normals(ctx, nPoints, xyz.data(), nviews.data(), viewIds.data(), 16, nrm.data()));
	if (o.estimateColors == 0) bgr.clear();
	if (o.estimateNormals == 0) nrm.clear();
	const double tFused = now_s();
	if (o.verbosity > 1)
		printf("Depth-maps fused and filtered: %zu depth-maps, %llu depths, %llu points (%d%%) in %.2f s (%.2f Mpoints/s)\n", order.size(),
		       (unsigned long long)nDepths, (unsigned long long)nPoints, nDepths ? (int)std::lround(100.0 * nPoints / nDepths) : 0, tFused - tCopied,
		       nPoints / (tFused - tCopied) / 1e6);
	// the scene and the point cloud, side by side
	const std::string base = o.output.substr(0, o.output.rfind('.'));
	bool okMvs = false, okPly = false;
	{
		std::thread tm([&] { okMvs = save_mvs(o.output, platforms, mimages, xyz, nrm, bgr, nviews, viewIds, viewWeights); });
		okPly = save_ply(base + ".ply", xyz, nrm, bgr);
		tm.join();
	}
	if (!okMvs || !okPly) { fprintf(stderr, "error: can not write the output files\n"); return EXIT_FAILURE; }
	if (!wait_files()) return EXIT_FAILURE;
	if (o.verbosity > 1) printf("Scene, point cloud and depth-maps saved (%.2f s after the fusion); total %.2f s\n", now_s() - tFused, now_s() - tStart);
	release_all();
	return EXIT_SUCCESS;
}
