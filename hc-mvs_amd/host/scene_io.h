/*
 * hc-mvs_amd/host/scene_io.h -- the files DensifyPointCloud reads and writes, and the image helpers that go with them: `.mvs` scenes
 * (MVSI v3-5, Interface.h:363-619), binary PPM / PGM images and label images, raw 'DR' depth maps (Interface.h:634-652), PLY point clouds;
 * cv::resize's INTER_AREA and INTER_CUBIC as the reference uses them, and the working size of an image at a resolution level.
 * Header-only like ply_mesh.h: plain C++, nothing but the standard library, no HIP.
 */
#ifndef HCMVS_SCENE_IO_H
#define HCMVS_SCENE_IO_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace sceneio {

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
inline bool load_mvs(const std::string& path, std::vector<MvsPlatform>& platforms, std::vector<MvsImage>& images, std::vector<Vertex>& verts,
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
inline bool save_mvs(const std::string& path, const std::vector<MvsPlatform>& platforms, const std::vector<MvsImage>& images,
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
inline bool pnm_header(std::ifstream& f, int& w, int& h, int& ch, int* maxvOut = nullptr) { // maxvOut: any maxval, reported
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
inline bool load_labels(const std::string& path, int& w, int& h, std::vector<uint16_t>& lab) {
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
inline bool pnm_size(const std::string& path, int& w, int& h) {
	std::ifstream f(path, std::ios::binary);
	int ch;
	return f && pnm_header(f, w, h, ch);
}
inline bool load_pnm(const std::string& path, int& w, int& h, std::vector<uint8_t>& bgr) {
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
inline void resize_area_bgr(int& w, int& h, std::vector<uint8_t>& bgr, int nw, int nh) {
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
#ifdef _OPENMP // (the driver is built with OpenMP; the header also compiles without)
#pragma omp parallel for schedule(static)
#endif
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
inline void working_size(int w, int h, unsigned level, unsigned minSize, unsigned maxSize, int& nw, int& nh) {
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

// raw 'DR' file (Interface.h:634-652): any of depth (flag 1), normal (2), confidence (4); null = not stored.  What the file says about its
// image: name, id, size, camera (K, R, C), the scene image ids of its source views, depth range
struct DmapImage { const std::string& name; uint32_t id; int w, h; const double *K, *R, *C; const std::vector<uint32_t>& srcIds; float dMin, dMax; };
inline bool save_dmap(const std::string& path, const DmapImage& im, const float* d, const float* n, const float* c) {
	std::ofstream f(path + ".tmp", std::ios::binary); // atomic like DepthData::Save (DepthMap.cpp:253-286)
	if (!f) return false;
	struct __attribute__((packed)) Hdr { uint16_t name; uint8_t type, pad; uint32_t iw, ih, dw, dh; float dMin, dMax; } h;
	const size_t px = (size_t)im.w * im.h;
	h.name = 0x5244; h.type = (uint8_t)((d ? 1 : 0) | (n ? 2 : 0) | (c ? 4 : 0)); h.pad = 0; h.iw = h.dw = (uint32_t)im.w; h.ih = h.dh = (uint32_t)im.h; h.dMin = im.dMin; h.dMax = im.dMax;
	f.write((const char*)&h, 28);
	const uint16_t nl = (uint16_t)im.name.size();
	f.write((const char*)&nl, 2); f.write(im.name.data(), nl);
	const uint32_t nids = 1 + (uint32_t)im.srcIds.size();
	f.write((const char*)&nids, 4); f.write((const char*)&im.id, 4); f.write((const char*)im.srcIds.data(), (std::streamsize)im.srcIds.size() * 4);
	f.write((const char*)im.K, 72); f.write((const char*)im.R, 72); f.write((const char*)im.C, 24);
	if (d) f.write((const char*)d, (std::streamsize)px * 4);
	if (n) f.write((const char*)n, (std::streamsize)px * 12);
	if (c) f.write((const char*)c, (std::streamsize)px * 4);
	f.close();
	return (bool)f && std::rename((path + ".tmp").c_str(), path.c_str()) == 0;
}
inline bool save_ply(const std::string& path, const RawArray<float>& xyz, const RawArray<float>& nrm, const RawArray<uint8_t>& bgr) {
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
inline bool load_dmap(const std::string& path, DmapFile& m, int what, bool headerOnly = false) {
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
inline void resize_cubic(const std::vector<float>& src, int sw, int sh, int ch, std::vector<float>& dst, int dw, int dh) {
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

inline std::string dirname_of(const std::string& p) { const size_t k = p.find_last_of('/'); return k == std::string::npos ? "." : p.substr(0, k); }
inline std::string map_path(const std::string& dir, const char* fmt, uint32_t id) { char nm[96]; snprintf(nm, sizeof nm, fmt, id); return dir + nm; }

} // namespace sceneio

#endif
