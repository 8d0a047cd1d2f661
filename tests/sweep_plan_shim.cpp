// C face of hc-mvs_amd/csrc/sweep_plan.h for tests/test_sweep_plan.py (ctypes).  Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/sweep_plan.h"

using namespace hcmvs;

static void put_variant(const SweepVariant& v, int* out) {
	const int f[8] = {v.nw, v.big, v.two, v.pack, v.hint, v.mask, v.spread, sweep_variant_exists(v)};
	for (int i = 0; i < 8; ++i) out[i] = f[i];
}

extern "C" {
int sp_segments_for(int V) { return segments_for(V); }
int sp_exists(int nw, int big, int two, int pack, int hint, int mask, int spread) {
	return sweep_variant_exists({nw, big != 0, two != 0, pack != 0, hint != 0, mask != 0, spread != 0});
}
// out[8]: nw, big, two, pack, hint, mask, spread, exists
void sp_resolve(int requested, int V, int big, int hint, int mask, int spread, int* out) {
	put_variant(resolve_sweep_variant(requested, V, big != 0, hint != 0, mask != 0, spread != 0), out);
}
// items: n x (rows, cols, nSrc, hintLast, mask, spread); knobs: sweepPerLaunch, sweepSegment, wavesPerRow.
// out: per launch (first, count, segLen, tickets, grid, then as sp_resolve), 13 ints, at most cap launches.  Returns the length of the plan.
int sp_plan(const int* items, int n, int big, int nSweeps, int nCU, const int* knobs, int* out, int cap) {
	SweepBatch b;
	for (int i = 0; i < n; ++i, items += 6) b.items.push_back({items[0], items[1], items[2], items[3] != 0, items[4] != 0, items[5] != 0});
	b.big = big != 0; b.nSweeps = nSweeps; b.nCU = nCU;
	b.sweepPerLaunch = knobs[0]; b.sweepSegment = knobs[1]; b.wavesPerRow = knobs[2];
	const std::vector<SweepLaunch> plan = plan_sweeps(b);
	for (int i = 0; i < (int)plan.size() && i < cap; ++i, out += 13) {
		const SweepLaunch& l = plan[i];
		out[0] = l.first; out[1] = l.count; out[2] = l.segLen; out[3] = l.tickets; out[4] = l.grid;
		put_variant(l.v, out + 5);
	}
	return (int)plan.size();
}
}
