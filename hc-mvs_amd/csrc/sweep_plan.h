/*
 * hc-mvs_amd/csrc/sweep_plan.h -- how a batch's sweeps are launched: which kernel instance, how many launches, what a ticket is.
 * Host policy only, plain C++17 without a HIP header, so that tests/test_sweep_plan.py checks it on a CPU.  plan_sweeps() is the
 * one place that decides; launch_sweep (pm_kernels.hip) launches what a SweepLaunch says and nothing else.
 */
#ifndef HCMVS_SWEEP_PLAN_H
#define HCMVS_SWEEP_PLAN_H

#include <stdlib.h>
#include <string.h>
#include <vector>

namespace hcmvs {

// lane layout class of an estimate with V source views (the items of a batch must share it).  Every estimate runs the 8 view groups
// x 8 tap segments layout: once for up to 8 views (class 8), twice for 9..16 (class 4: two sets of eight view groups, TWO in the
// kernels); view counts that leave groups idle let them work on (hypothesis, view) pairs of their own (PACK)
constexpr int segments_for(int V) { return V <= 8 ? 8 : 4; }
// a view count that leaves two or more of a set's eight view groups idle takes the variant whose idle groups work on
// (hypothesis, view) pairs of their own (score_chunk PACK; with one idle group it costs more than it saves)
constexpr bool view_count_packs(int V) { return V % 8 != 0 && V % 8 != 7; }

constexpr int kSweepGridCap = 8192;  // one workgroup per ticket; tickets beyond the grid are picked up by the workgroups that finish
constexpr int kSweepStretch = 256;   // columns of an automatic stretch
constexpr int kSweepStretchMin = 32; // (the ring of a row's latest results is re-read from memory at the start of a stretch)

// one instance of sweep_kernel<8, NW, BIG, TWO, PACK, HINT, MASK, SPREAD, PRIOR, GEO>
struct SweepVariant {
	int nw; // waves per row
	bool big, two, pack, hint, mask, spread;
	bool prior = false; // some item of the launch has an active depth prior
	bool geo = false;   // some item of the launch has the geometric-consistency term active
};
// THE set of sweep instances the library holds (248: 152 without the prior term, 48 with it -- a prior comes without the hint and
// without view spread -- and 48 with the geometric-consistency term, which comes without the hint, view spread and the prior, so a GEO
// instance exists exactly where the PRIOR instance of the same shape does): the launcher's table is generated from this predicate, so
// nothing else is compiled and nothing else can be launched
constexpr bool sweep_variant_exists(SweepVariant v) {
	return v.nw >= 1 && v.nw <= 4 && (v.nw <= 2 || !(v.big || v.hint)) && (v.nw <= 3 || !v.spread) && (!v.prior || !(v.hint || v.spread)) &&
	       (!v.geo || !(v.hint || v.spread || v.prior));
}
// The instance for `requested` waves per row in a launch whose selecting item has V source views (plan_sweeps: vSel).  Patches beyond
// 64 taps and the one sweep of a run that carries the hint run with one or two waves per row; a launch with view spread has no
// four-wave instance (three waves compute the same maps); a request outside 1..4 gets two.
constexpr SweepVariant resolve_sweep_variant(int requested, int V, bool big, bool hint, bool mask, bool spread, bool prior = false, bool geo = false) {
	int nw = 2;
	if (big || hint) nw = requested >= 2 ? 2 : 1;
	else if (requested == 1 || requested == 3) nw = requested;
	else if (requested == 4) nw = spread ? 3 : 4;
	return {nw, big, V > 8, view_count_packs(V), hint, mask, spread, prior, geo};
}

struct SweepItem {
	int rows, cols, nSrc;   // H - 2 * border, W - 2 * border, source views
	bool hintLast;          // offers the `restore` variant's extra hypothesis in the last sweep
	bool mask, spread;      // has a keep-mask (EstConst::keep), has view spread to do (EstConst::spread)
	bool prior = false;     // has an active depth prior (PriorItem::prior)
	bool geo = false;       // has the geometric-consistency term active (GeoItem::views)
};
struct SweepBatch {
	std::vector<SweepItem> items;
	bool big = false;       // patches beyond 64 taps (adapthalfwin > kHalfWindow)
	int nSweeps = 0;
	int firstSweep = 0;     // index of the batch's first sweep (hcmvs_estimate_sweeps_batch_device: the sweeps go on where an estimate ended)
	int nCU = 0;            // compute units of the device; <= 0: 256
	int sweepPerLaunch = 0; // HCMVS_SWEEP_LAUNCHES: 0 automatic, 1 per-sweep, 2 one
	int sweepSegment = -1;  // HCMVS_SWEEP_SEGMENT: columns per ticket; -1 automatic, 0 whole rows
	int wavesPerRow = 0;    // HCMVS_WAVES_PER_ROW: 1..4; 0 automatic
};
// The tuning knobs of the environment as a context holds them.  Each argument is the variable's text, null when it is unset; a text
// that does not spell one of the accepted values leaves the default, silently.
struct SweepKnobs {
	int lag = 1;        // HCMVS_SWEEP_LAG: columns a row starts behind the previous one; a number >= 1
	int affinity = 1;   // HCMVS_XCD_AFFINITY: rows of an image prefer the workgroups of one XCD; any number, 0 turns it off
	int perLaunch = 0;  // HCMVS_SWEEP_LAUNCHES: "per-sweep" 1, "one" 2 (SweepBatch::sweepPerLaunch)
	int segment = -1;   // HCMVS_SWEEP_SEGMENT: columns per ticket, a number >= 0 (SweepBatch::sweepSegment)
	int wavesPerRow = 0; // HCMVS_WAVES_PER_ROW: 1, 2, 3 or 4 (SweepBatch::wavesPerRow)
};
inline SweepKnobs parse_sweep_knobs(const char* lag, const char* affinity, const char* launches, const char* segment, const char* waves) {
	SweepKnobs k;
	if (lag && atoi(lag) >= 1) k.lag = atoi(lag);
	if (affinity) k.affinity = atoi(affinity) != 0;
	if (launches && strcmp(launches, "per-sweep") == 0) k.perLaunch = 1;
	if (launches && strcmp(launches, "one") == 0) k.perLaunch = 2;
	if (segment && atoi(segment) >= 0) k.segment = atoi(segment);
	if (waves && atoi(waves) >= 1 && atoi(waves) <= 4) k.wavesPerRow = atoi(waves);
	return k;
}
// One launch for the sweeps first .. first + count - 1 of every item (indices as the kernel sees them: SweepBatch::firstSweep included) (tickets, rowsDone and the progress words of the items must be zero)
struct SweepLaunch {
	int first, count;
	SweepVariant v;  // hint: some item offers its hint in one of these sweeps; mask / spread / prior / geo: some item has a keep-mask / view spread to do / an active prior / the geometric-consistency term active
	int segLen;      // > 0: a ticket is a stretch of segLen columns of a row; 0: a whole row
	int tickets, grid;
};

inline std::vector<SweepLaunch> plan_sweeps(const SweepBatch& b) {
	int totalRows = 0;
	bool hintLast = false, mask = false, spread = false, prior = false, geo = false;
	// the kernel variant goes by view count: an item whose count leaves two or more view groups idle wants the pair-packing variant,
	// which is correct for the other items of its layout class too
	int vSel = b.items.empty() ? 0 : b.items[0].nSrc;
	for (const SweepItem& it : b.items) {
		totalRows += it.rows;
		hintLast = hintLast || it.hintLast; mask = mask || it.mask; spread = spread || it.spread; prior = prior || it.prior; geo = geo || it.geo;
		if (view_count_packs(it.nSrc)) vSel = it.nSrc;
	}
	// Waves per row, by how the batch's rows compare with the workers the chip holds at once (12 per CU: 4 SIMDs x 3 sweep workers; the
	// big-patch worker: two waves per SIMD; measured on 1080p images, profiles/r04_launch_modes.txt): a batch of few rows is bound by
	// the latency of one pixel along the (W + H) critical path of its row wavefronts, and the scoring of a pixel's hypotheses divides
	// among the waves of a row -- three waves for one image (1066 rows), two for two or three (a lone 3840x2160 image has 2146 rows:
	// two), one from there on, where the chip's throughput counts.  More waves than workers are fine since the rows are handed out in
	// stretches (below): a row no longer needs a worker of its own from its first to its last column.
	const int slots = (b.nCU > 0 ? b.nCU : 256) * (b.big ? 8 : 12);
	const int requested = b.wavesPerRow ? b.wavesPerRow : (10 * totalRows <= 4 * slots ? 3 : (10 * totalRows <= 11 * slots ? 2 : 1));
	// A batch whose rows fill the chip four times over (12 images of 1080p or more) runs all its sweeps in ONE launch (round 4): the images go
	// through their sweeps independently of each other, without a chip-wide drain and refill between two sweeps (+5 % at 12, +7 % at 16 images,
	// +2.6 ... 3.5 % at 32; profiles/r04_launch_modes.txt).  Fewer images are bound by the latency of their row wavefronts, not by the
	// chip, and gain nothing from it (measured: 4 -> 8 % slower), so they keep one launch per sweep.
	const bool perSweep = b.sweepPerLaunch == 1 || (b.sweepPerLaunch == 0 && totalRows < 4 * slots);
	std::vector<SweepLaunch> plan;
	for (int first = 0; first < b.nSweeps;) {
		int count = perSweep ? 1 : b.nSweeps - first;
		// The `restore` variant's extra hypothesis belongs to the last sweep of the last outer iteration: that sweep gets a launch of its
		// own, with the kernel instance that knows the hint.
		bool hint = false;
		if (hintLast) { if (first == b.nSweeps - 1) hint = true; else if (first + count == b.nSweeps) --count; }
		// A launch of ONE sweep with more waves than the chip holds workers (and less than four times as many rows: from there on all
		// sweeps run in one launch) hands out stretches of 256 columns instead of whole rows: a worker's slot comes free after 256 pixels.
		// With whole rows the rows beyond the resident set begin only when row 0 has reached its end -- 8 images: 107.2 -> 100.3 ms per
		// sweep; it is also what lets one to three images have two or three waves per row (1: 35.6 -> 33.7 ms, 2: 46.1 -> 42.0,
		// 3: 59.9 -> 55.4); 4 and 5 images: 0 ... +2 % (profiles/r04_launch_modes.txt).
		// The rule counts the REQUESTED waves, the kernel runs with the resolved ones (a hint or big-patch launch asked for 3 runs 2, and
		// still goes in stretches where 2 * totalRows <= slots).  The maps are the same either way; which is faster is not measured
		// (last item) and is left to a change that measures it.
		SweepLaunch l{b.firstSweep + first, count, resolve_sweep_variant(requested, vSel, b.big, hint, mask, spread, prior, geo), 0, totalRows, 0};
		if (b.sweepSegment > 0 || (b.sweepSegment < 0 && count == 1 && requested * totalRows > slots && totalRows < 4 * slots)) {
			l.segLen = b.sweepSegment > 0 ? b.sweepSegment : kSweepStretch;
			if (l.segLen < kSweepStretchMin) l.segLen = kSweepStretchMin;
			l.tickets = 0;
			for (const SweepItem& it : b.items) l.tickets += it.rows * ((it.cols + l.segLen - 1) / l.segLen);
		}
		l.grid = l.tickets < kSweepGridCap ? l.tickets : kSweepGridCap;
		plan.push_back(l);
		first += count;
	}
	return plan;
}

} // namespace hcmvs
#endif
