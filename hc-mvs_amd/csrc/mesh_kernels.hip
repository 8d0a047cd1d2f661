/*
 * hc-mvs_amd/csrc/mesh_kernels.hip -- uniform point sampling of a triangle mesh on the device.
 *
 * Mesh::SamplePoints (frame_main/libs/MVS/Mesh.cpp:3444-3527, DensifyPointCloud --sample-mesh) walks the faces in order: face f of area
 * A_f gets (unsigned)(A_f * density) points and one more with the probability of the fractional part; every point is Turk's uniform
 * triangle sample O + x u + y v with (x, y) folded across the diagonal when x + y > 1; with a texture the point takes the bilinear
 * sample at the interpolated texture coordinate.  The reference draws from a std::mt19937 seeded by std::random_device -- sequential and
 * not reproducible.  Here the draws are counter-based: draw k of face f under seed s is
 *   U = (mix(mix(s ^ mix(f)) + k * 0xD1B54A32D192ED03) >> 11) * 2^-53,    mix = the splitmix64 step,
 * draw 0 decides the extra point (U <= fractional part), point i of the face uses draws 1 + 2 i and 2 + 2 i.  The cloud depends on
 * (mesh, sample, seed) only and comes out in the reference's order: faces ascending, the points of a face in draw order.
 *
 * Three launches: one thread per face (float area, count), an exclusive scan of the counts (hipcub), one thread per point
 * (upper-bound search of its face in the offsets -- neighbouring lanes share a face, so its loads broadcast --, the two draws, the point,
 * optionally the face index and the colour).  The host waits only for the total count and, for --sample-mesh < 0, for the float areas:
 * Mesh::ComputeArea sums them into a double one after the other in face order, and that sum is taken on the host exactly so.
 * Arithmetic: edges, cross product and the point in float32 with every product rounded (no contraction), norm(u x v) * 0.5 in double,
 * as the reference has them.  The point pass is bound by its stores (19 B per point).
 */
#include "mesh_kernels.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <exception>
#include <vector>

namespace hcmvs {

namespace {

static const dim3 kBlock(256);
constexpr unsigned long long kMaxCount = 1ull << 32; // per face: a face with more refuses the call (fewer than 2^32 points in all)

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
// a = mix(seed ^ mix(face)) is the face's stream
__device__ __forceinline__ double draw(unsigned long long a, unsigned long long k) {
	return (double)(mix64(a + k * 0xD1B54A32D192ED03ull) >> 11) * 0x1p-53;
}
struct Tri { float O[3], u[3], v[3]; };
__device__ __forceinline__ void load_tri(const float* vertices, const uint32_t* faces, unsigned long long f, Tri& t) {
	const float* O = vertices + 3 * (size_t)faces[3 * f];
	const float* A = vertices + 3 * (size_t)faces[3 * f + 1];
	const float* B = vertices + 3 * (size_t)faces[3 * f + 2];
#pragma unroll
	for (int q = 0; q < 3; ++q) { t.O[q] = O[q]; t.u[q] = A[q] - O[q]; t.v[q] = B[q] - O[q]; }
}

// one thread per face.  areaF (or null): ComputeTriangleArea<float> (Util.inl:476-482), what Mesh::ComputeArea sums; withCounts: the count of
// the face, from its double area (kept in a register: nothing else reads it), and the zero-area tally.  --sample-mesh < 0 runs the kernel
// twice, for the float areas and, once the density is known, for the counts: recomputing a cross product is cheaper than storing and
// reloading 8 B per face
__global__ __launch_bounds__(256) void face_kernel(unsigned long long nFaces, const float* vertices, const uint32_t* faces, double density, unsigned long long seed,
                                                   int withCounts, float* areaF, unsigned long long* counts, unsigned long long* zeroFaces) {
	unsigned long long zero = 0;
	for (unsigned long long f = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; f < nFaces; f += (unsigned long long)gridDim.x * blockDim.x) {
		Tri t;
		load_tri(vertices, faces, f, t);
		const float cx = t.u[1] * t.v[2] - t.u[2] * t.v[1], cy = t.u[2] * t.v[0] - t.u[0] * t.v[2], cz = t.u[0] * t.v[1] - t.u[1] * t.v[0];
		if (areaF) areaF[f] = sqrtf(((cx * cx + cy * cy) + cz * cz) / 4.f);
		if (!withCounts) continue;
		const double area = sqrt(((double)cx * (double)cx + (double)cy * (double)cy) + (double)cz * (double)cz) * 0.5; // cv::norm(Point3f): double
		const double fp = area * density;
		unsigned long long n = fp < 4294967296.0 ? (unsigned long long)fp : (fp != fp ? 0ull : kMaxCount);
		const double frac = fp - (double)n;
		if (draw(mix64(seed ^ mix64(f)), 0) <= frac) ++n;
		counts[f] = n;
		zero += area == 0.0;
	}
	if (withCounts) {
		for (int o = 32; o > 0; o >>= 1) zero += __shfl_xor(zero, o, 64);
		if ((threadIdx.x & 63) == 0 && zero) atomicAdd(zeroFaces, zero);
		if (blockIdx.x == 0 && threadIdx.x == 0) counts[nFaces] = 0; // the scan runs over nFaces + 1 items: offsets[nFaces] is the total
	}
}

// float -> int32: truncating, saturating, NaN -> 0 (the reference's (int) casts, defined for every input)
__device__ __forceinline__ int sat_int(float v) {
	if (v != v) return 0;
	if (v >= 2147483648.f) return 2147483647;
	if (v <= -2147483648.f) return (int)0x80000000;
	return (int)v;
}
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(unsigned)sat_int(v); }

struct Texture { const uint8_t* bgr; int w, h; };
// TImage::getPixel (Types.inl:2232-2243): coordinates clamped to the image
__device__ __forceinline__ const uint8_t* get_pixel(const Texture& t, long long y, long long x) {
	x = x < 0 ? 0 : (x >= t.w ? t.w - 1 : x);
	y = y < 0 ? 0 : (y >= t.h ? t.h - 1 : y);
	return t.bgr + 3 * ((size_t)y * t.w + (size_t)x);
}

// one thread per point
__global__ __launch_bounds__(256) void point_kernel(unsigned long long nPoints, unsigned long long nFaces, const float* vertices, const uint32_t* faces,
                                                    const unsigned long long* offsets, unsigned long long seed, const float* texcoords, Texture tex,
                                                    float* xyz, uint32_t* faceOf, uint8_t* bgr) {
	for (unsigned long long p = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; p < nPoints; p += (unsigned long long)gridDim.x * blockDim.x) {
		// the face: the last f with offsets[f] <= p (offsets[0] == 0, offsets[nFaces] == nPoints > p; empty faces repeat an offset)
		unsigned long long lo = 0, hi = nFaces;
		while (hi - lo > 1) { const unsigned long long mid = (lo + hi) >> 1; if (offsets[mid] <= p) lo = mid; else hi = mid; }
		const unsigned long long f = lo, i = p - offsets[f];
		const unsigned long long a = mix64(seed ^ mix64(f));
		double x = draw(a, 1 + 2 * i), y = draw(a, 2 + 2 * i);
		if (x + y > 1.0) { x = 1.0 - x; y = 1.0 - y; }
		const float fx = (float)x, fy = (float)y;
		Tri t;
		load_tri(vertices, faces, f, t);
#pragma unroll
		for (int q = 0; q < 3; ++q) xyz[3 * p + q] = (t.O[q] + fx * t.u[q]) + fy * t.v[q];
		if (faceOf) faceOf[p] = (uint32_t)f;
		if (bgr) {
			const float* T = texcoords + 6 * f; // TO, TA, TB
			const float xtx = (T[0] + fx * (T[2] - T[0])) + fy * (T[4] - T[0]), xty = (T[1] + fx * (T[3] - T[1])) + fy * (T[5] - T[1]);
			const float px = xtx * (float)tex.w, py = (1.f - xty) * (float)tex.h;
			// TImage::sampleSafe (Types.inl:2261-2269); Pixel8U arithmetic goes back to 8 bits at every step (Types.h:1930-1937)
			const int lx = sat_int(px), ly = sat_int(py);
			const float sx = px - (float)lx, sx1 = 1.f - sx, sy = py - (float)ly, sy1 = 1.f - sy;
			const uint8_t *p00 = get_pixel(tex, ly, lx), *p01 = get_pixel(tex, ly, (long long)lx + 1), *p10 = get_pixel(tex, (long long)ly + 1, lx),
			              *p11 = get_pixel(tex, (long long)ly + 1, (long long)lx + 1);
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				const uint8_t top = to_u8((float)(uint8_t)(to_u8(sx1 * (float)p00[k]) + to_u8(sx * (float)p01[k])) * sy1);
				const uint8_t bot = to_u8((float)(uint8_t)(to_u8(sx1 * (float)p10[k]) + to_u8(sx * (float)p11[k])) * sy);
				bgr[3 * p + k] = (uint8_t)(top + bot);
			}
		}
	}
}
} // namespace

namespace {
int sample_mesh_impl(const MeshSampleInput& in, unsigned long long capacity, float* hXyz, uint32_t* hFaceOf, uint8_t* hBgr, bool wantArea, MeshSampleCounters& st,
                     Reclaimer* rec, hipStream_t s, std::string& err) {
	st = MeshSampleCounters();
	const unsigned long long nF = in.nFaces;
	const bool needArea = in.sample < 0 || wantArea; // the positive form needs the mesh area for the counters only
	std::vector<float> hArea(needArea ? nF : 0);          // may throw: before anything that would have to be undone
	const bool textured = in.texture && in.texcoords;
	const size_t texBytes = textured ? (size_t)in.texW * (size_t)in.texH * 3 : 0;
	size_t scanBytes = 0;
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(nF + 1));
	Carve carve;
	const size_t oV = carve((size_t)in.nVertices * 12), oF = carve(nF * 12), oAf = carve(nF * 4), oCnt = carve((nF + 1) * 8),
	             oOff = carve((nF + 1) * 8), oT = carve(textured ? nF * 24 : 0), oTex = carve(texBytes), oZero = carve(64), oScan = carve(scanBytes);
	auto fits = [&](size_t bytes) { // against the free device memory, after giving back what the context can spare
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return true; }
		if (bytes > freeB && rec && rec->reclaim() && hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return true; }
		return bytes <= freeB;
	};
	char msg[160];
	if (!fits(carve.size)) {
		snprintf(msg, sizeof msg, "sample_mesh: the mesh needs %.1f MiB of device memory, more than is free", carve.size / 1048576.0);
		err = msg;
		return 1;
	}
	DevBuf work(rec), out(rec); // freed on return
	if (work.reserve(carve.size, s) != hipSuccess) { err = "sample_mesh: out of device memory"; return 2; }
	char* b = work.get();
	st.deviceBytes = carve.size;
	hipEvent_t ev[2] = {nullptr, nullptr};
	auto fail = [&](const char* what) {
		err = what;
		(void)hipStreamSynchronize(s); // work and out are freed on return
		(void)hipGetLastError();
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
		return 2;
	};
	auto done = [&](int rc) { for (auto& e : ev) if (e) (void)hipEventDestroy(e); return rc; };
	if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) return fail("sample_mesh: event creation failed");
	float *dV = (float*)(b + oV), *areaF = (float*)(b + oAf), *dT = textured ? (float*)(b + oT) : nullptr;
	uint32_t* dF = (uint32_t*)(b + oF);
	unsigned long long *counts = (unsigned long long*)(b + oCnt), *offsets = (unsigned long long*)(b + oOff), *zero = (unsigned long long*)(b + oZero);
	if (hipMemcpyAsync(dV, in.vertices, (size_t)in.nVertices * 12, hipMemcpyHostToDevice, s) != hipSuccess ||
	    hipMemcpyAsync(dF, in.faces, nF * 12, hipMemcpyHostToDevice, s) != hipSuccess || hipMemsetAsync(zero, 0, 64, s) != hipSuccess)
		return fail("sample_mesh: upload failed");
	if (textured && (hipMemcpyAsync(dT, in.texcoords, nF * 24, hipMemcpyHostToDevice, s) != hipSuccess ||
	                 hipMemcpyAsync(b + oTex, in.texture, texBytes, hipMemcpyHostToDevice, s) != hipSuccess))
		return fail("sample_mesh: upload failed");
	(void)hipEventRecord(ev[0], s);
	const dim3 faceGrid((unsigned)std::min<unsigned long long>((nF + 255) / 256, 8192));
	auto total_area = [&]() { // Mesh::ComputeArea (Mesh.cpp:3423-3429): REAL area += float, face after face
		double a = 0;
		for (unsigned long long f = 0; f < nF; ++f) a += hArea[f];
		return a;
	};
	double density = (double)in.sample;
	if (in.sample < 0) { // Mesh::SamplePoints(unsigned) (Mesh.cpp:3444-3454): density = numberOfPoints / ComputeArea()
		hipLaunchKernelGGL(face_kernel, faceGrid, kBlock, 0, s, nF, dV, dF, 0.0, in.seed, 0, areaF, counts, zero);
		if (hipGetLastError() != hipSuccess) return fail("sample_mesh: launch failed");
		if (hipMemcpyAsync(hArea.data(), areaF, nF * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
			return fail("sample_mesh: device failure");
		st.area = total_area();
		const unsigned n = (unsigned)(int)std::floor(-in.sample + .5f); // ROUND2INT = Round2Int(float): int(floor(x + .5f)), in float (Types.h:937-943)
		if (st.area < (double)0.0001f) return done(0);                         // ZEROTOLERANCE<float>(): an empty cloud
		density = (double)n / st.area;
	}
	st.density = density;
	hipLaunchKernelGGL(face_kernel, faceGrid, kBlock, 0, s, nF, dV, dF, density, in.seed, 1, in.sample > 0 && needArea ? areaF : (float*)nullptr, counts, zero);
	if (hipGetLastError() != hipSuccess) return fail("sample_mesh: launch failed");
	if (hipcub::DeviceScan::ExclusiveSum(b + oScan, scanBytes, counts, offsets, (int)(nF + 1), s) != hipSuccess) return fail("sample_mesh: scan failed");
	unsigned long long total = 0, hZero = 0;
	if (hipMemcpyAsync(&total, offsets + nF, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(&hZero, zero, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    (in.sample > 0 && needArea && hipMemcpyAsync(hArea.data(), areaF, nF * 4, hipMemcpyDeviceToHost, s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess)
		return fail("sample_mesh: device failure");
	if (in.sample > 0 && needArea) st.area = total_area();
	st.zeroAreaFaces = hZero;
	st.points = total;
	if (total >= kMaxCount) { err = "sample_mesh: 2^32 points or more"; return done(1); }
	if (!hXyz || total == 0) { (void)hipEventRecord(ev[1], s); (void)hipEventSynchronize(ev[1]); (void)hipEventElapsedTime(&st.ms, ev[0], ev[1]); return done(0); }
	if (total > capacity) {
		snprintf(msg, sizeof msg, "sample_mesh: room for %llu points, %llu needed", capacity, total);
		err = msg;
		return done(1);
	}
	const bool wantFace = hFaceOf != nullptr, wantBgr = hBgr != nullptr && textured;
	Carve oc;
	const size_t oX = oc(total * 12), oFo = oc(wantFace ? total * 4 : 0), oB = oc(wantBgr ? total * 3 : 0);
	if (!fits(oc.size)) { // refused before the point pass is launched
		snprintf(msg, sizeof msg, "sample_mesh: %llu points need %.1f MiB of device memory, more than is free", total, oc.size / 1048576.0);
		err = msg;
		return done(1);
	}
	if (out.reserve(oc.size, s) != hipSuccess) return fail("sample_mesh: out of device memory");
	st.deviceBytes += oc.size;
	char* ob = out.get();
	float* dX = (float*)(ob + oX);
	uint32_t* dFo = wantFace ? (uint32_t*)(ob + oFo) : nullptr;
	uint8_t* dB = wantBgr ? (uint8_t*)(ob + oB) : nullptr;
	const Texture tex{textured ? (const uint8_t*)(b + oTex) : nullptr, in.texW, in.texH};
	hipLaunchKernelGGL(point_kernel, dim3((unsigned)std::min<unsigned long long>((total + 255) / 256, 65536)), kBlock, 0, s, total, nF, dV, dF, offsets, in.seed, dT,
	                   tex, dX, dFo, dB);
	if (hipGetLastError() != hipSuccess) return fail("sample_mesh: launch failed");
	(void)hipEventRecord(ev[1], s);
	if (hipMemcpyAsync(hXyz, dX, total * 12, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    (wantFace && hipMemcpyAsync(hFaceOf, dFo, total * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
	    (wantBgr && hipMemcpyAsync(hBgr, dB, total * 3, hipMemcpyDeviceToHost, s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess)
		return fail("sample_mesh: device failure");
	(void)hipEventElapsedTime(&st.ms, ev[0], ev[1]);
	return done(0);
}
} // namespace

// the host side allocates (4 B per face, the messages): an allocation that fails must not leave through the C entry as an exception
int sample_mesh_device(const MeshSampleInput& in, unsigned long long capacity, float* xyz, uint32_t* faceOfPoint, uint8_t* bgr, bool wantArea, MeshSampleCounters& st,
                       Reclaimer* rec, hipStream_t s, std::string& err) {
	try {
		return sample_mesh_impl(in, capacity, xyz, faceOfPoint, bgr, wantArea, st, rec, s, err);
	} catch (const std::exception&) {
		(void)hipStreamSynchronize(s);
		try { err = "sample_mesh: out of host memory"; } catch (...) {}
		return 2;
	}
}

} // namespace hcmvs
