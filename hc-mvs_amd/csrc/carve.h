/* hc-mvs_amd/csrc/carve.h -- the carving of one allocation into pieces: plain C++ (no HIP), for dev_buf.h and the host-side plans */
#ifndef HCMVS_CARVE_H
#define HCMVS_CARVE_H
#include <stddef.h>
namespace hcmvs {

// Offsets of the pieces of one allocation, each rounded up to 256 bytes; size is what the allocation needs
struct Carve {
	size_t size = 0;
	size_t operator()(size_t bytes) { const size_t o = size; size += (bytes + 255) & ~(size_t)255; return o; }
};

} // namespace hcmvs
#endif
