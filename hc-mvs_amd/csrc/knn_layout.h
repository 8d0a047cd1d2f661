/* hc-mvs_amd/csrc/knn_layout.h -- the pieces of the k-nearest-neighbour index (knn_grid.h) inside one allocation: plain C++ (no HIP), so
 * that the host-side plans can lay their scratch out around it */
#ifndef HCMVS_KNN_LAYOUT_H
#define HCMVS_KNN_LAYOUT_H
#include <stddef.h>
#include "carve.h"
namespace hcmvs {

struct KnnLayout { size_t keys = 0, keys2 = 0, idx = 0, idx2 = 0, sorted = 0, pos = 0, box = 0, sort = 0, sortBytes = 0; };

// n points; sortBytes: what the radix sort of n (key 8 B, value 4 B) pairs asks for as temporary storage
inline KnnLayout knn_layout(Carve& carve, size_t n, size_t sortBytes) {
	KnnLayout l;
	l.sortBytes = sortBytes;
	l.keys = carve(n * 8); l.keys2 = carve(n * 8); l.idx = carve(n * 4); l.idx2 = carve(n * 4); l.sorted = carve(n * 16); l.pos = carve(n * 4); l.box = carve(64);
	l.sort = carve(sortBytes);
	return l;
}

} // namespace hcmvs
#endif
