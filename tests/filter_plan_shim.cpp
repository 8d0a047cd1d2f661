// C face of hc-mvs_amd/csrc/filter_plan.h for tests/test_filter_plan.py (ctypes).  Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/filter_plan.h"

using namespace hcmvs;

extern "C" {
// returns 1 and the cap when the text is a valid HCMVS_FILTER_BATCH (text may be NULL), else 0
int fp_parse(const char* text, unsigned long long nImages, unsigned long long* cap) {
	size_t c = 0;
	const bool ok = parse_filter_batch(text, (size_t)nImages, &c);
	*cap = c;
	return ok ? 1 : 0;
}
// first: room for n + 1 entries; returns the number of entries written (batches + 1), *keyBytes the keys of the largest batch
int fp_plan(const unsigned long long* need, int n, unsigned long long budget, unsigned long long cap, unsigned long long* first, unsigned long long* keyBytes) {
	const FilterPlan p = plan_filter_batches(std::vector<size_t>(need, need + n), (size_t)budget, (size_t)cap);
	for (size_t i = 0; i < p.first.size(); ++i) first[i] = p.first[i];
	*keyBytes = p.keyBytes;
	return (int)p.first.size();
}
// the allocation of a plan fails whenever it needs more than `avail` bytes: the plans tried, as the entry point's loop tries them.
// Returns the number of allocations attempted (at most maxTries), *keyBytes the plan that fitted, or 0 when the call gives up.
int fp_retry(const unsigned long long* need, int n, unsigned long long budget, unsigned long long cap, unsigned long long avail, int maxTries, unsigned long long* keyBytes) {
	const std::vector<size_t> nd(need, need + n);
	size_t b = (size_t)budget;
	*keyBytes = 0;
	for (int t = 1; t <= maxTries; ++t) {
		const FilterPlan p = plan_filter_batches(nd, b, (size_t)cap);
		if (p.keyBytes <= avail) { *keyBytes = p.keyBytes; return t; }
		b = filter_retry_budget(nd, p);
		if (!b) return t;
	}
	return maxTries + 1;
}
}
