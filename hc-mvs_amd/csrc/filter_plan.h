/* hc-mvs_amd/csrc/filter_plan.h -- how hcmvs_filter_sequence cuts its images into batches: plain C++ (no HIP), so that
 * tests/test_filter_plan.py checks it without a GPU. */
#ifndef HCMVS_FILTER_PLAN_H
#define HCMVS_FILTER_PLAN_H
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
namespace hcmvs {

// HCMVS_FILTER_BATCH: "all" or a positive decimal number, nothing else.  cap = images per batch (0: text == NULL, by memory alone)
inline bool parse_filter_batch(const char* text, size_t nImages, size_t* cap) {
	*cap = 0;
	if (!text) return true;
	if (!strcmp(text, "all")) { *cap = nImages ? nImages : 1; return true; }
	char* end = nullptr;
	const long v = strtol(text, &end, 10);
	if (end == text || *end != '\0' || v < 1) return false;
	*cap = (size_t)v;
	return true;
}

struct FilterPlan {
	std::vector<size_t> first; // first image of every batch, then the number of images
	size_t keyBytes = 0;       // z-buffer keys of the largest batch
};
// need[k]: key bytes of image k.  Consecutive images share a batch until the next one would take it beyond `budget` bytes or `cap`
// images (0: no cap); an image larger than the budget gets a batch of its own.
inline FilterPlan plan_filter_batches(const std::vector<size_t>& need, size_t budget, size_t cap) {
	FilterPlan p;
	p.first.assign(1, 0);
	size_t cur = 0;
	for (size_t k = 0; k < need.size(); ++k) {
		if (k > p.first.back() && (need[k] > budget || cur > budget - need[k] || (cap && k - p.first.back() >= cap))) { p.first.push_back(k); cur = 0; }
		cur += need[k];
		p.keyBytes = std::max(p.keyBytes, cur);
	}
	p.first.push_back(need.size());
	return p;
}
// The keys of plan p could not be allocated: the budget to plan with next, or 0 when no plan needs less -- the largest batch is
// already down to the largest single image.  A plan made with the returned budget has keyBytes <= max(largest image, p.keyBytes / 2)
// < p.keyBytes, so retrying ends.
inline size_t filter_retry_budget(const std::vector<size_t>& need, const FilterPlan& p) {
	size_t largest = 0;
	for (size_t n : need) largest = std::max(largest, n);
	if (p.keyBytes <= largest) return 0;
	return std::max<size_t>(p.keyBytes / 2, 1);
}

} // namespace hcmvs
#endif
