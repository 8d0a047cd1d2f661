/* hc-mvs_amd/csrc/mesh_kernels.h -- uniform point sampling of a triangle mesh on the device (mesh_kernels.hip) */
#ifndef HCMVS_MESH_KERNELS_H
#define HCMVS_MESH_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "dev_buf.h"
namespace hcmvs {
struct MeshSampleInput {
	uint32_t nVertices = 0, nFaces = 0;
	const float* vertices = nullptr;    // nVertices * 3, finite
	const uint32_t* faces = nullptr;    // nFaces * 3, every index < nVertices
	const float* texcoords = nullptr;   // nFaces * 6 or null
	const uint8_t* texture = nullptr;   // texH * texW * 3 (B,G,R) or null
	int texW = 0, texH = 0;
	float sample = 0.f;                 // > 0: points per square unit, < 0: -(number of points)
	unsigned long long seed = 0;
};
struct MeshSampleCounters {
	unsigned long long zeroAreaFaces = 0, points = 0, deviceBytes = 0;
	double area = 0, density = 0;
	float ms = 0.f;
};
// Mesh::SamplePoints (Mesh.cpp:3444-3527) with the counter-based draws of DESIGN.md section 5 (D11).  Host arrays in and out; xyz == null:
// only st.points is computed.  faceOfPoint / bgr: optional outputs (bgr needs a texture).  wantArea: st.area also for sample > 0 (a copy
// of 4 B per face and a sum on the host that the sampling itself does not need; sample < 0 always has it).  The caller has validated the mesh.
// 0 = ok, 1 = refused (2^32 points or more, capacity too small -- st.points says what is needed --, output larger than the free device
// memory), 2 = device failure (err says which)
int sample_mesh_device(const MeshSampleInput& in, unsigned long long capacity, float* xyz, uint32_t* faceOfPoint, uint8_t* bgr, bool wantArea, MeshSampleCounters& st,
                       Reclaimer* rec, hipStream_t s, std::string& err);
}
#endif
