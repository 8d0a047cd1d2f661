/*
 * hc-mvs_amd/host/driver_plan.h -- every decision of a DensifyPointCloud run that needs no device, each stated once: the option table and
 * what is derived from it, the cameras and the view selection, how the reference images are dealt to the devices, what has to fit into a
 * device, the batches, which thread does what in which outer iteration, and how large the cloud's buffers are.  The driver
 * (DensifyPointCloud.cpp) asks the device for its free memory and does what this header says; tests/test_driver_plan.py checks the
 * arithmetic on the CPU.  Plain C++, no HIP.
 */
#ifndef HCMVS_DRIVER_PLAN_H
#define HCMVS_DRIVER_PLAN_H

#include "../../include/hcmvs_hip.h"
#include "scene_io.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace driverplan {

using sceneio::MvsCamera;
using sceneio::MvsPose;
using sceneio::Vertex;

// ---- options ---------------------------------------------------------------------------------------------------------
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
	int postFilter = -1;          // --n-postfilter 0|1: override of that gate (-1: follow --n-nOptimize; parse_options resolves it to 0 or 1)
	int viewspread = 0;           // --n-viewspread 1: view spread (DepthMap.cpp:1504-1608).  The reference's default is 1; 0 here keeps
	                              // the results of every existing command line
	int postFilterInterleave = 0; // --n-postfilter-interleave 1: estimate(k) -> post-filter(k) -> estimate(k + 1), the reference's own order
	                              // (SceneDensify.cpp:3889-3965), one image per launch; 0: estimate all, then filter all
	int nFilter = 0;              // --n-filter 0|1|2: the depth-map filter stage before the fusion (Scene::DenseReconstructionFilter, SceneDensify.cpp:4100-4185, which the
	                              // fork switched off with if(0) at :3721): 0 off, 1 adjust (bFilterAdjust = 1), 2 strict.  --n-nOptimize bit 4 (ADJUST_FILTER) stays inert
	int resume = 1;               // skip-if-exists (SceneDensify.cpp:3865-3880): an image whose final depth map is already in the working folder is not estimated again
	int restoreHypothesis = 0;    // 1: the `restore` binary's extra last-sweep hypothesis from the previous level's maps
	                              // (restore/libs/MVS/DepthMap.cpp:1527-1549); needs the previous level's maps in the working folder
	std::string depthPriors;      // --depth-priors <folder>: per image a raw 'DR' depth map depth%04u.prior.dmap (the name the commented-out export at
	                              // SceneDensify.cpp:3990-3991 would give) of the image's size at the run's resolution level; only the depth is read;
	                              // an image without a file has no prior (DepthMap.cpp:941-954)
	float paraPrior = 0.5f, sigmaPrior = 0.2f; // --n-para_prior, --sigma-prior (DensifyPointCloud.cpp:183, :162)
	int photo2geo = 2;            // --n-photo2geo (DensifyPointCloud.cpp:175): first outer iteration that blends the prior term
	int geoConsistency = 0;       // --geo-consistency 1: the geometric-consistency term: from outer iteration max(1, --n-photo2geo)
	                              // on every view score is blended with a reprojection term against the source views' maps of the previous outer iteration
	float paraTapa = 0.25f;       // --n-para_tapa (DensifyPointCloud.cpp:176-181): the term's weight where the pixel has low texture
	float paraTapa2 = 0.15f;      // --n-para_tapa2: ... medium texture
	float txThreshold = 150.f;    // --n-txthreshold: the texture threshold of --n-para_tapa
	float txThreshold2 = 160.f;   // --n-txthreshold2: the texture threshold of --n-para_tapa2
	float geoMaxPx = 3.f;         // --geo-max-px: the reprojection error, in pixels, at and beyond which a pair is "worst"
	int planePriors = 0;          // --plane-priors 1: the priors are GENERATED on outer iteration n - 2 from planes fitted inside the pixels labelled 255 of
	                              // seman/<stem>.quad.pgm|ppm (hcmvs_generate_plane_prior_device); an image without a label file has none
	std::string exportPriors;     // --export-priors <dir>: every generated prior as <dir>/depth%04u.prior.dmap, the raw 'DR' form --depth-priors reads
	float ransacProbability = 0.01f, ransacEpsilon = 2.f, ransacMinPoints = 80.f; // --ransac-probability, --ransac-epsilon (eps = spacing x this),
	                              // --ransac-min-points (a plane has at least 1 / this of the fitting set): the parameters of the plane detection
	int planeClusters = 0;        // --plane-clusters 1 (with --plane-priors 1): a plane keeps the largest connected component of its inliers, on cells of
	                              // --ransac-cluster average spacings; 0 keeps the results of command lines written before it
	float ransacCluster = 10.f;   // --ransac-cluster (the reference's default; the authors run 7): read and unused without --plane-clusters 1
	int planeRefit = 0;           // --plane-refit n (with --plane-priors 1), 0 .. 16: least-squares steps on the winner of every round of the plane detection, over
	                              // its inliers in the eps / 4 band; 0 keeps the results of command lines written before it
	int speckleSize = 0;          // --speckle-size n: after the end pass of the last outer iteration the segments of fewer than n pixels are removed from every
	                              // finished depth map (hcmvs_remove_speckles_batch_device); upstream's nSpeckleSize is 100; 0 is off
	float speckleDiff = 0.01f * 0.7f; // --speckle-diff f: two neighbouring depths belong to one segment when they differ by less than f of either
	int device = 0, batch = 32;   // reference images per launch: 32 is the measured optimum (profiles/r02_knobs.txt); lowered when HBM is short
	std::vector<int> devices;     // --devices 0,1,...: one context + host thread per entry; reference images sharded over them by their position in
	                              // the fusion order (k mod N); post-filters and fusion on the first (an ordinal may repeat: two contexts on one GPU)
	uint32_t seed = 1234;
	int thFilterPointCloud = 0;   // --filter-point-cloud: < 0 filters the input scene's cloud by visibility and nothing else; >= 0: no effect, as in the reference
	float sampleMesh = 0.f;       // --sample-mesh: != 0 samples a cloud on the input mesh and nothing else; 0: no effect, as in the reference
	unsigned long long sampleSeed = 1234; // --seed as --sample-mesh takes it: all 64 bits
	std::vector<std::string> notes;      // accepted options that do nothing in this build, for the driver to print (-v > 1)
};

// every option of the reference's table (DensifyPointCloud.cpp:71-198) plus the ones of this driver; all take a value.
// Unknown options are an error (boost::program_options throws on them, DensifyPointCloud.cpp:222-233).
static const char* const kKnownOptions[] = {
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

// ... and the options that feed or make the depth priors (a table of its own: kKnownOptions is the reference's table plus the driver's first set)
static const char* const kPriorOptions[] = {"--depth-priors", "--plane-priors", "--export-priors"};
// ... and the switch of the inlier clustering of the generated priors (a third table: the two above are pinned as they are)
static const char* const kPlaneClusterOptions[] = {"--plane-clusters"};
// ... and the geometric-consistency term's own (a fourth table; --n-para_tapa, --n-para_tapa2, --n-txthreshold, --n-txthreshold2 and
// --n-photo2geo, which feed it, are the reference's and stand in kKnownOptions)
static const char* const kGeoOptions[] = {"--geo-consistency", "--geo-max-px"};
// ... and the refit of the winning plane of the generated priors (a fifth table, for the same reason as the third)
static const char* const kPlaneRefitOptions[] = {"--plane-refit"};
// ... and the speckle filter's two (a sixth table, for the same reason)
static const char* const kSpeckleOptions[] = {"--speckle-size", "--speckle-diff"};

static const char* const kUsage =
	"usage: DensifyPointCloud -i scene.mvs [-o out.mvs] [-w dir] [--resolution-level n] [--number-views n] "
	"[--n-EstimationIters n] [--n-EstimationIters-external n] [--n-adapthalfwin n] [--fusion-mode 0|1] ...\n"
	"       --n-viewspread 0|1   from outer iteration 1 on every pixel also tries what its source views' depth maps hold where it projects to\n"
	"                            (default 0; the reference's default is 1 -- 0 keeps the results of command lines written before it existed)\n"
	"       --depth-priors <dir> prior depth maps, <dir>/depth%04u.prior.dmap per image (raw 'DR' depth map of the image's size at the run's resolution\n"
	"                            level; an image without a file has none), blended into every score with --n-para_prior, --sigma-prior and\n"
	"                            --n-photo2geo; registered on outer iteration n - 2 with two extra sweeps, kept through the last.  Not together with\n"
	"                            --n-viewspread 1 or --restore-hypothesis 1\n"
	"       --geo-consistency 0|1  geometric consistency: from outer iteration max(1, --n-photo2geo) on every view score is blended with a reprojection\n"
	"                            term against the source view's own depth and normal map of the previous outer iteration, with the weight\n"
	"                            --n-para_tapa where the pixel's texture is below --n-txthreshold, --n-para_tapa2 where it is below --n-txthreshold2;\n"
	"                            --geo-max-px (default 3) is the error at which a pair counts as worst (default 0; --n-usegeoconsistency, the fork's dead\n"
	"                            blend, stays unavailable).  One device.  Not together with --n-viewspread 1, --restore-hypothesis 1, --depth-priors or\n"
	"                            --plane-priors 1\n"
	"       --plane-priors 0|1   generate the priors instead: on outer iteration n - 2 planes are fitted inside the pixels labelled 255 of\n"
	"                            seman/<stem>.quad.pgm|ppm of every image that has one (--ransac-probability, --ransac-epsilon, --ransac-min-points and\n"
	"                            --seed feed the detection) and rendered into the image's prior; from there as --depth-priors.  --export-priors <dir>\n"
	"                            writes them as <dir>/depth%04u.prior.dmap.  Not together with --depth-priors, --n-viewspread 1 or --restore-hypothesis 1\n"
	"       --plane-clusters 0|1 with --plane-priors 1: a plane keeps only the largest connected component of its inliers, on a grid of cells of\n"
	"                            --ransac-cluster average spacings (default 10) in the plane, so that two coplanar surfaces with something else between\n"
	"                            them become two planes (default 0: --ransac-cluster is read and unused, the results of earlier command lines)\n"
	"       --plane-refit n      with --plane-priors 1: the winning plane of every round of the detection is refitted by n least-squares steps over its\n"
	"                            inliers within a quarter of the --ransac-epsilon band, before its inliers are assigned or clustered (0 .. 16; default 0:\n"
	"                            the plane is the best of the candidates spanned by three samples, the results of earlier command lines)\n"
	"       --speckle-size n     the speckle filter: after the last outer iteration every finished depth map loses its segments of fewer than n pixels\n"
	"                            (4-neighbours are of one segment when their depths differ by less than --speckle-diff of either, default 0.01 x 0.7);\n"
	"                            upstream OpenMVS runs it with nSpeckleSize 100.  The .dmap files, --n-filter and the fusion see the filtered maps\n"
	"                            (default 0: off, the results of earlier command lines)\n"
	"       --n-filter 0|1|2     the depth-map filter stage before the fusion: every depth map against up to 8 neighbours' maps (0 off, the default;\n"
	"                            1 adjust: consistent depths are averaged, 2 strict: kept as they are); the final .dmap files hold the filtered maps\n"
	"                            (with --resume 1 a second run loads those filtered maps and filters them again, as the reference would)\n"
	"       DensifyPointCloud -i dense.mvs [-o out.mvs] --filter-point-cloud <negative threshold>   (visibility filter of the cloud only:\n"
	"       writes <out>_filtered.mvs and <out>_filtered.ply)\n"
	"       DensifyPointCloud -i mesh.ply [-o out.mvs] --sample-mesh <d> [--seed n]   (samples a point cloud on a PLY triangle mesh and writes\n"
	"       <out>.ply: d > 0 points per square unit, d < 0 minus the number of points; colours when the mesh is textured by a binary PPM)\n";

enum ParseResult { PARSE_OK = 0, PARSE_USAGE = 1, PARSE_ERROR = 2 };

// The command line into `o`, with everything derived from it: postFilter from the --n-nOptimize bits, the defaults of the working folder and
// the output, and -- for a densify run -- the batch within [1, HCMVS_MAX_BATCH] and at least one outer iteration.  PARSE_ERROR: `err` is the
// message; PARSE_USAGE: no input file or -h (kUsage).  The checks of a densify run (--fusion-mode, --n-filter) do not apply to
// --sample-mesh / --filter-point-cloud runs, which read neither.  o.notes is filled as far as the parse got.
inline ParseResult parse_options(int argc, char** argv, Options& o, std::string& err) {
	std::map<std::string, std::string> kv;
	for (int i = 1; i < argc; ++i) {
		std::string a = argv[i], val;
		if (a == "-h" || a == "--help") { kv["--help"] = "1"; continue; }
		const size_t eq = a.find('=');
		bool haveVal = false;
		if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); haveVal = true; }
		bool known = false;
		for (const char* k : kKnownOptions) known = known || a == k;
		for (const char* k : kPriorOptions) known = known || a == k;
		for (const char* k : kPlaneClusterOptions) known = known || a == k;
		for (const char* k : kGeoOptions) known = known || a == k;
		for (const char* k : kPlaneRefitOptions) known = known || a == k;
		for (const char* k : kSpeckleOptions) known = known || a == k;
		if (!known) { err = "unrecognised option '" + a + "'"; return PARSE_ERROR; }
		if (!haveVal) { // the value is the next argument, whatever it starts with (negative numbers are values)
			if (i + 1 >= argc) { err = "the required argument for option '" + a + "' is missing"; return PARSE_ERROR; }
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
	geti("--fuse-order", o.fuseOrder); geti("--fuse-count", o.fuseCount); geti("--restore-hypothesis", o.restoreHypothesis); geti("--n-postfilter", o.postFilter);
	geti("--n-postfilter-interleave", o.postFilterInterleave); geti("--n-nOptimize", o.nOptimize); geti("--resume", o.resume); geti("--n-viewspread", o.viewspread);
	geti("--n-filter", o.nFilter);
	getf("--n-para_prior", o.paraPrior); getf("--sigma-prior", o.sigmaPrior); geti("--n-photo2geo", o.photo2geo);
	if (kv.count("--depth-priors")) o.depthPriors = kv["--depth-priors"];
	geti("--plane-priors", o.planePriors);
	if (kv.count("--export-priors")) o.exportPriors = kv["--export-priors"];
	getf("--ransac-probability", o.ransacProbability); getf("--ransac-epsilon", o.ransacEpsilon); getf("--ransac-min-points", o.ransacMinPoints);
	geti("--plane-clusters", o.planeClusters); getf("--ransac-cluster", o.ransacCluster);
	geti("--plane-refit", o.planeRefit);
	geti("--speckle-size", o.speckleSize); getf("--speckle-diff", o.speckleDiff);
	geti("--geo-consistency", o.geoConsistency); getf("--geo-max-px", o.geoMaxPx);
	getf("--n-para_tapa", o.paraTapa); getf("--n-para_tapa2", o.paraTapa2); getf("--n-txthreshold", o.txThreshold); getf("--n-txthreshold2", o.txThreshold2);
	geti("--device", o.device); geti("--batch", o.batch);
	if (kv.count("--devices")) { // comma-separated HIP ordinals
		std::stringstream ss(kv["--devices"]);
		std::string tok;
		while (std::getline(ss, tok, ',')) {
			if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) { err = "--devices expects a comma-separated list of device ordinals"; return PARSE_ERROR; }
			o.devices.push_back(atoi(tok.c_str()));
		}
		if (o.devices.empty() || o.devices.size() > 64) { err = "--devices expects 1 to 64 device ordinals"; return PARSE_ERROR; }
	} else o.devices.push_back(o.device);
	o.device = o.devices[0];
	if (kv.count("--seed")) o.seed = (uint32_t)strtoul(kv["--seed"].c_str(), nullptr, 10);
	o.sampleSeed = kv.count("--seed") ? strtoull(kv["--seed"].c_str(), nullptr, 10) : (unsigned long long)o.seed;
	geti("--estimate-colors", o.estimateColors); geti("--estimate-normals", o.estimateNormals);
	geti("--max-resolution", o.maxResolution); geti("--min-resolution", o.minResolution);
	if (o.postFilter < 0) o.postFilter = (o.nOptimize & 3) != 0 ? 1 : 0; // OPTDENSE::OPTIMIZE = REMOVE_SPECKLES | FILL_GAPS (DepthMap.h:113-118)
	for (const char* k : {"--n-opticalflow", "--use-semantic", "--n-usegeoconsistency", "--n-usepartconsistency"})
		if (kv.count(k) && atoi(kv[k].c_str()) != 0 && o.verbosity > 1)
			o.notes.push_back(std::string(k) + " is not available in this build (defined subset); treated as 0" +
			                  (std::string(k) == "--use-semantic" ? " (prior depth maps made elsewhere can be supplied with --depth-priors <folder>)" : ""));
	geti("--filter-point-cloud", o.thFilterPointCloud);
	getf("--sample-mesh", o.sampleMesh);
	if (o.input.empty() || kv.count("--help")) return PARSE_USAGE;
	if (o.workdir.empty()) o.workdir = sceneio::dirname_of(o.input);
	if (o.output.empty()) o.output = o.input.substr(0, o.input.rfind('.')) + "_dense.mvs";
	if (o.sampleMesh != 0 || o.thFilterPointCloud < 0) return PARSE_OK; // (no densify run)
	if (o.fusionMode < 0) { err = "SGM fusion modes are not available"; return PARSE_ERROR; }
	if (o.nFilter < 0 || o.nFilter > 2) { err = "--n-filter expects 0 (off), 1 (adjust) or 2 (strict)"; return PARSE_ERROR; }
	if (o.planePriors != 0 && o.planePriors != 1) { err = "--plane-priors expects 0 or 1"; return PARSE_ERROR; }
	if (!o.exportPriors.empty() && !o.planePriors) { err = "--export-priors writes the priors that --plane-priors 1 generates: give both"; return PARSE_ERROR; }
	if (o.planeClusters != 0 && o.planeClusters != 1) { err = "--plane-clusters expects 0 or 1"; return PARSE_ERROR; }
	if (o.planeClusters && !o.planePriors) { err = "--plane-clusters 1 clusters the inliers of the planes that --plane-priors 1 fits: give both"; return PARSE_ERROR; }
	if (o.speckleSize < 0) { err = "--speckle-size expects a number of pixels >= 0 (0 is off; upstream's nSpeckleSize is 100)"; return PARSE_ERROR; }
	if (!(o.speckleDiff > 0.f) || !(o.speckleDiff < INFINITY)) { err = "--speckle-diff expects a finite value > 0"; return PARSE_ERROR; }
	if (o.planeRefit < 0 || o.planeRefit > 16) { err = "--plane-refit expects a number of steps from 0 to 16"; return PARSE_ERROR; }
	if (o.planeRefit && !o.planePriors) { err = "--plane-refit refits the planes that --plane-priors 1 fits: give both"; return PARSE_ERROR; }
	if (o.planePriors) {
		if (!o.depthPriors.empty()) { err = "--plane-priors 1 is not combined with --depth-priors (an image has one prior: generated or supplied)"; return PARSE_ERROR; }
		if (o.restoreHypothesis) { err = "--plane-priors 1 is not combined with --restore-hypothesis 1 (the prior term does not come with the hint)"; return PARSE_ERROR; }
		if (o.viewspread) { err = "--plane-priors 1 is not combined with --n-viewspread 1 (the authors run priors with --n-viewspread 0)"; return PARSE_ERROR; }
		if (!(o.ransacProbability > 0.f && o.ransacProbability < 1.f)) { err = "--ransac-probability expects a value inside (0, 1)"; return PARSE_ERROR; }
		if (!(o.ransacEpsilon > 0.f) || !(o.ransacEpsilon < INFINITY)) { err = "--ransac-epsilon expects a finite value > 0"; return PARSE_ERROR; }
		if (!(o.ransacMinPoints > 0.f) || !(o.ransacMinPoints < INFINITY)) { err = "--ransac-min-points expects a finite value > 0"; return PARSE_ERROR; }
		if (o.planeClusters && (!(o.ransacCluster > 0.f) || !(o.ransacCluster < INFINITY))) { err = "--ransac-cluster expects a finite value > 0 (with --plane-clusters 1)"; return PARSE_ERROR; }
		if (!o.planeClusters && kv.count("--ransac-cluster") && o.verbosity > 1)
			o.notes.push_back("--ransac-cluster is read and unused: the plane detection does not cluster a plane's inliers into connected components (--plane-clusters 1 does)");
	}
	if (!o.depthPriors.empty() || o.planePriors) { // (without either the three prior options are read and have nothing to act on)
		if (!o.depthPriors.empty() && o.restoreHypothesis) { err = "--depth-priors is not combined with --restore-hypothesis 1 (the prior term does not come with the hint)"; return PARSE_ERROR; }
		if (!o.depthPriors.empty() && o.viewspread) { err = "--depth-priors is not combined with --n-viewspread 1 (the authors run priors with --n-viewspread 0)"; return PARSE_ERROR; }
		if (!(o.paraPrior >= 0.f && o.paraPrior <= 1.f)) { err = "--n-para_prior expects a value in [0, 1]"; return PARSE_ERROR; }
		if (!(o.sigmaPrior > 0.f) || !(o.sigmaPrior < INFINITY)) { err = "--sigma-prior expects a finite value > 0"; return PARSE_ERROR; }
		if (o.photo2geo < 0) { err = "--n-photo2geo expects a value >= 0"; return PARSE_ERROR; }
	}
	if (o.geoConsistency != 0 && o.geoConsistency != 1) { err = "--geo-consistency expects 0 or 1"; return PARSE_ERROR; }
	if (o.geoConsistency) { // (without it the options that feed the term are read and have nothing to act on)
		if (o.viewspread) { err = "--geo-consistency 1 is not combined with --n-viewspread 1 (the library refuses the term together with view spread at work)"; return PARSE_ERROR; }
		if (o.restoreHypothesis) { err = "--geo-consistency 1 is not combined with --restore-hypothesis 1 (the term does not come with the hint)"; return PARSE_ERROR; }
		if (!o.depthPriors.empty()) { err = "--geo-consistency 1 is not combined with --depth-priors (the term does not come with the prior term)"; return PARSE_ERROR; }
		if (o.planePriors) { err = "--geo-consistency 1 is not combined with --plane-priors 1 (the term does not come with the prior term)"; return PARSE_ERROR; }
		if (!(o.paraTapa >= 0.f && o.paraTapa <= 1.f)) { err = "--n-para_tapa expects a value in [0, 1]"; return PARSE_ERROR; }
		if (!(o.paraTapa2 >= 0.f && o.paraTapa2 <= 1.f)) { err = "--n-para_tapa2 expects a value in [0, 1]"; return PARSE_ERROR; }
		if (!(fabsf(o.txThreshold) < INFINITY) || !(fabsf(o.txThreshold2) < INFINITY)) { err = "--n-txthreshold and --n-txthreshold2 expect finite values"; return PARSE_ERROR; }
		if (!(o.geoMaxPx > 0.f) || !(o.geoMaxPx < INFINITY)) { err = "--geo-max-px expects a finite value > 0"; return PARSE_ERROR; }
		if (o.photo2geo < 0) { err = "--n-photo2geo expects a value >= 0"; return PARSE_ERROR; }
	}
	if (o.batch < 1) o.batch = 1;
	if (o.batch > HCMVS_MAX_BATCH) o.batch = HCMVS_MAX_BATCH;
	if (o.estimationItersExternal < 1) o.estimationItersExternal = 1;
	return PARSE_OK;
}

// ---- cameras and views (Camera.h) ------------------------------------------------------------------------------------
struct Camera { double K[9], R[9], C[3]; };
// what the host knows about an image of the scene; the driver adds the pixels and the device maps
struct PlanImage {
	std::string name;
	uint32_t id = 0;
	int w = 0, h = 0;
	Camera cam;
	bool valid = false;
	std::vector<uint32_t> points;               // sparse points seen (>= 2 views), Scene.cpp:568-569
	struct Nb { uint32_t id; uint32_t points; float scale, angle, area, score; };
	std::vector<Nb> neighbors;                  // Scene.cpp:640-650, sorted by score
	std::vector<uint32_t> srcs;                 // SceneDensify.cpp:362-367 (the ids the estimate is called with: resampled copies get ids of their own)
	std::vector<float> srcScale;                // per source view: 1 or the scale it is resampled by (ViewData::ScaleImage)
	size_t pixels() const { return (size_t)w * h; }
};

inline void mat3mul(const double* a, const double* b, double* c) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j]; c[i * 3 + j] = s; }
}
inline void w2c(const Camera& c, const float* X, double* o) {
	const double d[3] = {X[0] - c.C[0], X[1] - c.C[1], X[2] - c.C[2]};
	for (int i = 0; i < 3; ++i) o[i] = c.R[i * 3] * d[0] + c.R[i * 3 + 1] * d[1] + c.R[i * 3 + 2] * d[2];
}
// the camera of an image at the size w x h: Interface.h:451-459 pose composition (R = Rcam Rpose, C = Rpose^T Ccam + Cpose) and
// Scene.cpp:83-91 + Camera.h:167-180 (GetK): K normalised by max(w,h) of the camera, scaled to w x h
inline void image_camera(const MvsCamera& c, const MvsPose& q, int w, int h, Camera& cam) {
	mat3mul(c.R, q.R, cam.R);
	for (int k = 0; k < 3; ++k) cam.C[k] = q.R[0 * 3 + k] * c.C[0] + q.R[1 * 3 + k] * c.C[1] + q.R[2 * 3 + k] * c.C[2] + q.C[k];
	const double s = (double)std::max(w, h) / (c.w && c.h ? (double)std::max(c.w, c.h) : 1.0);
	memcpy(cam.K, c.K, sizeof cam.K);
	cam.K[1] = 0;
	cam.K[0] *= s; cam.K[4] *= s;
	if (c.K[2] == 0 && c.K[5] == 0) { cam.K[2] = 0.5 * (w - 1); cam.K[5] = 0.5 * (h - 1); }
	else { cam.K[2] *= s; cam.K[5] *= s; }
}
inline bool project(const Camera& c, const float* X, float& u, float& v, double& z) {
	double p[3];
	w2c(c, X, p);
	z = p[2];
	if (p[2] <= 0) return false;
	u = (float)(c.K[2] + c.K[0] * p[0] / p[2]); v = (float)(c.K[5] + c.K[4] * p[1] / p[2]);
	return true;
}

// Scene.cpp:545-661 SelectNeighborViews + Scene.cpp:665-678 FilterNeighborViews (defaults DepthMap.cpp:69-143).  Image: PlanImage or
// what the driver derives from it; fills points, neighbors, srcs and srcScale of images[ID] and reads cameras and sizes of the others
template <typename Image>
bool select_views(std::vector<Image>& images, const std::vector<Vertex>& verts, uint32_t ID, int nMaxViews, int numberViews) {
	typedef PlanImage::Nb Nb;
	PlanImage& A = images[ID];
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
			const PlanImage& B = images[w.first];
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
		const PlanImage& B = images[IDB];
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
		Nb nb{IDB, s.points, s.avgScale / s.points, s.avgAngle / s.points, cells / 256.f, 0.f};
		nb.score = s.score * nb.area;
		A.neighbors.push_back(nb);
	}
	std::stable_sort(A.neighbors.begin(), A.neighbors.end(), [](const Nb& a, const Nb& b) { return a.score > b.score; });
	if (A.points.size() <= 3 || A.neighbors.size() < (size_t)std::min<int>(2, (int)images.size() - 1)) return false;
	std::vector<Nb> kept;
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

// ---- dealing the reference images to the devices ---------------------------------------------------------------------------
// The order of the fusion and of the post-filters' fusion: best connected images first (SceneDensify.cpp:3285-3302).  It also deals the
// reference images to the devices: position k of it goes to device k mod N, so that the devices are loaded alike.
// needGray[d][i]: device d needs the gray image of scene image i -- every image on one device; on several, a device's own reference
// images and their source views only.  (The first device also gets camera + colour image of every other image, because it filters and
// fuses the whole scene.)  To be called while srcs still holds scene image ids.
struct Deal {
	std::vector<uint32_t> fuseOrder;
	std::vector<int> dev;                    // by image id; 0 for an image that is not in `todo`
	std::vector<std::vector<char>> needGray; // [device][image id]
};
template <typename Image>
Deal plan_deal(const std::vector<Image>& images, const std::vector<uint32_t>& todo, int nDev) {
	Deal deal;
	deal.fuseOrder = todo;
	std::stable_sort(deal.fuseOrder.begin(), deal.fuseOrder.end(), [&](uint32_t a, uint32_t b) { return images[a].neighbors.size() > images[b].neighbors.size(); });
	deal.dev.assign(images.size(), 0);
	for (size_t k = 0; k < deal.fuseOrder.size(); ++k) deal.dev[deal.fuseOrder[k]] = (int)(k % (size_t)nDev);
	deal.needGray.assign((size_t)nDev, std::vector<char>(images.size(), nDev > 1 ? 0 : 1));
	if (nDev > 1)
		for (uint32_t id : todo) {
			deal.needGray[(size_t)deal.dev[id]][id] = 1;
			for (uint32_t s : images[id].srcs) deal.needGray[(size_t)deal.dev[id]][s] = 1;
		}
	return deal;
}
// the neighbour list a map is registered with for the post-filters, the filter stage and the fusion: the scene neighbours that have maps
// (the ones in `todo`), at most 31
inline std::vector<uint32_t> registered_neighbors(const PlanImage& im, const std::vector<uint32_t>& todo) {
	std::vector<uint32_t> nb;
	for (const auto& x : im.neighbors) if (std::find(todo.begin(), todo.end(), x.id) != todo.end()) nb.push_back(x.id);
	if (nb.size() > 31) nb.resize(31);
	return nb;
}

// ---- the cloud's buffers -----------------------------------------------------------------------------------------------
// Before the fusion: the worst case.  A fused point claims at least number-views-fuse pixels (half a point per pixel from 2 on), and a
// point merges at most one depth per image (one view entry per pixel).
struct CloudSize { uint64_t capacity = 0, viewCapacity = 0; };
template <typename Image>
CloudSize cloud_worst_case(const std::vector<Image>& images, const std::vector<uint32_t>& todo, int numberViewsFuse) {
	CloudSize c;
	for (uint32_t id : todo) {
		const size_t n = images[id].pixels();
		c.capacity += (uint64_t)(numberViewsFuse >= 2 ? n / 2 : n);
		c.viewCapacity += (uint64_t)n;
	}
	return c;
}
// That worst case is 31 B per point + 8 B per view entry on the device and as much on the host: 166 GB for 512 images of 3840x2160.  A large
// scene is therefore fused twice: a counting pass first (no cloud; a fusion repeated on the maps a fusion has left makes the same decisions,
// so the second pass produces the cloud the first one counted), then the real one with buffers of exactly the size needed.
// --fuse-count 1 / 0 forces / forbids the counting pass.
inline bool fusion_counts_first(const CloudSize& worst, int fuseCount) {
	return ((worst.capacity * 31 + worst.viewCapacity * 8) > ((uint64_t)4 << 30) || fuseCount == 1) && fuseCount != 0;
}
// The memory budget asks the same question before anything is uploaded, and NOT with the same formula: it takes the worst case as 39 B per
// pixel of the scene whatever --number-views-fuse is, and --fuse-count 1 does not enter.  The two stay different here: making them one
// changes which scenes are refused and which batch is chosen.
inline bool budget_counts_first(size_t allPx, int fuseCount) { return allPx * 39 > ((size_t)4 << 30) && fuseCount != 0; }
// the device copy of the cloud in the budget: counted first, what is reserved is what the cloud holds -- taken as 0.2 points per pixel (the
// reference reserves 0.15, SceneDensify.cpp:3298) with 3 view entries each; otherwise half a point per pixel (31 B) + 8 B per view entry
inline size_t budget_cloud_bytes(size_t allPx, int fuseCount) {
	return budget_counts_first(allPx, fuseCount) ? allPx / 5 * (31 + 3 * 8) : allPx / 2 * 31 + allPx * 8;
}

// ---- what has to fit into a device ---------------------------------------------------------------------------------------
// Bytes per pixel of an image: resident per reference image of the device -- maps 20, hint maps 16 (restore variant), gray + colour +
// gradient 8; per source view the 2 x 2 footprints 16; per image of a batch the working state 24.  With --n-filter the first device also
// holds the stage's staging slabs and one image's z-buffer keys.  The first device also holds colour + gradient (4) and, with several
// devices, a copy of the maps (20) of EVERY image, the per-pass tables of the fusion (12 B per pixel and neighbour of the largest image +
// 40 B per pixel) and the device copy of the cloud.  The batch is halved until the device fits; `fits` is false when it does not at one
// image per launch (DESIGN.md section 4 has configs[3] in numbers).
struct DeviceBudget {
	size_t resident = 0, perImage = 0; // bytes that stay; bytes per image of a batch (the largest image's working state)
	int batch = 0;                     // what o.batch becomes on this device by halving
	bool fits = false;
	size_t ownImages = 0;              // reference images of the device
	size_t needed() const { return resident + (size_t)batch * perImage; }
};
template <typename Image>
DeviceBudget plan_device_budget(const std::vector<Image>& images, const std::vector<uint32_t>& todo, const Deal& deal, int d, size_t freeBytes, const Options& o) {
	const int nDev = (int)deal.needGray.size();
	size_t maxPx = 0, allPx = 0, ownPx = 0, grayPx = 0, maxNb = 1;
	DeviceBudget b;
	for (uint32_t id : todo) {
		const size_t px = images[id].pixels();
		maxPx = std::max(maxPx, px); allPx += px;
		if (deal.dev[id] == d) { ownPx += px; ++b.ownImages; }
		maxNb = std::max(maxNb, std::min<size_t>(images[id].neighbors.size(), 31));
	}
	for (size_t i = 0; i < images.size(); ++i) if (images[i].valid && deal.needGray[(size_t)d][i]) grayPx += images[i].pixels();
	b.resident = ownPx * (size_t)(20 + (o.restoreHypothesis ? 16 : 0)) + grayPx * (size_t)(8 + 16) + ((size_t)1 << 30);
	if (d == 0) {
		b.resident += allPx * 4 + (nDev > 1 ? allPx * 20 : 0) + maxPx * (12 * maxNb + 40);
		// --n-filter: the staging of the filtered maps (8 B per pixel of the scene) and the z-buffer keys of a batch of one image with 8
		// neighbours (the stage takes more images per batch when more memory is free)
		if (o.nFilter) b.resident += allPx * 8 + maxPx * 8 * 8;
		if (o.fusionMode != 1) b.resident += budget_cloud_bytes(allPx, o.fuseCount);
	}
	b.perImage = maxPx * 24;
	b.batch = o.batch;
	while (b.batch > 1 && b.needed() > freeBytes) b.batch /= 2;
	b.fits = b.needed() <= freeBytes;
	return b;
}

// ---- batches ---------------------------------------------------------------------------------------------------------
// Images of one device and one lane layout class (up to 8 source views, or 9..16) share a launch, `batch` at the most; the batches of the
// devices in turn (first batch of every device first), which is the order the loader serves them in.  work[d]: the images device d estimates
struct Batch { int dev; std::vector<uint32_t> ids; };
template <typename Image>
std::vector<Batch> plan_batches(const std::vector<Image>& images, const std::vector<std::vector<uint32_t>>& work, int batch) {
	std::vector<std::vector<Batch>> perDev(work.size());
	for (size_t d = 0; d < work.size(); ++d) {
		std::map<int, std::vector<uint32_t>> byClass;
		for (uint32_t id : work[d]) byClass[images[id].srcs.size() <= 8 ? 8 : 16].push_back(id);
		for (auto& g : byClass)
			for (size_t b0 = 0; b0 < g.second.size(); b0 += (size_t)batch)
				perDev[d].push_back(Batch{(int)d, std::vector<uint32_t>(g.second.begin() + (long)b0, g.second.begin() + (long)std::min(g.second.size(), b0 + (size_t)batch))});
	}
	std::vector<Batch> batches;
	for (size_t k = 0;; ++k) {
		bool any = false;
		for (size_t d = 0; d < work.size(); ++d) if (k < perDev[d].size()) { batches.push_back(perDev[d][k]); any = true; }
		if (!any) break;
	}
	return batches;
}

// ---- the schedule of an outer iteration -------------------------------------------------------------------------------------
// Every device context has a host thread (a worker) that estimates the context's batches; the main thread runs what needs all maps in one
// place.  With --n-nOptimize's REMOVE_SPECKLES | FILL_GAPS bits, after the estimates of outer iterations 1 and 2 every image goes through the
// post-filters (SceneDensify.cpp:3916, 3939-3958).  The interleaved schedule (--n-postfilter-interleave 1) runs such an iteration -- and,
// with view spread, every iteration >= 1 -- on the main thread, image after image.  The final maps go to the saver exactly once: by the
// worker, batch by batch, unless the last iteration ends on the main thread, which then hands them over itself; with --n-filter both leave
// it to the filter stage (the files hold the filtered maps).
struct IterPlan {
	bool filtered = false;            // the post-filters run after this iteration's estimates
	bool serial = false;              // the main thread estimates this iteration, one image per launch; the workers do not
	bool meet = false;                // the workers wait at the end of this iteration until the main thread lets them go (filtered or serial)
	bool snapshotSpread = false;      // view spread, batch schedule: the worker offers a copy of the maps as the previous iteration left them
	bool liveSpread = false;          // view spread, interleaved schedule: the main thread offers the live maps
	bool workerSubmitsFinal = false;  // the worker hands every batch it has estimated to the saver
	bool mainSubmitsFinal = false;    // the main thread hands the estimated images to the saver when the iteration is done
};
inline IterPlan plan_iteration(const Options& o, int it, bool anyWork) {
	const bool last = it == o.estimationItersExternal - 1;
	// (the source views offer their maps to view spread or to the geometric-consistency term: the same copies, the same registry)
	const bool filterNow = o.postFilter && (it == 1 || it == 2), spreadNow = (o.viewspread || o.geoConsistency) && it >= 1;
	IterPlan p;
	p.filtered = filterNow && anyWork;
	p.serial = o.postFilterInterleave && anyWork && (filterNow || spreadNow);
	p.meet = p.filtered || p.serial;
	p.snapshotSpread = spreadNow && !p.serial;
	p.liveSpread = spreadNow && p.serial;
	p.workerSubmitsFinal = last && anyWork && !p.meet && !o.nFilter;
	p.mainSubmitsFinal = last && p.meet && !o.nFilter;
	return p;
}
// --depth-priors, the reference's schedule (SceneDensify.cpp:983-1031): on outer iteration n - 2, after the ordinary estimate of a batch, the
// priors of its images are registered and two extra sweeps run (indices --n-EstimationIters and + 1); they stay registered through the last
// iteration.  With fewer than two outer iterations the priors are never used.
// --plane-priors 1 follows the same schedule: the priors are generated where --depth-priors registers the ones it read.
// --geo-consistency 1: the term's options as the library takes them
inline hcmvs_geo_params geo_params(const Options& o) {
	return {o.geoConsistency, o.paraTapa, o.paraTapa2, o.txThreshold, o.txThreshold2, o.photo2geo, o.geoMaxPx};
}
inline bool has_priors(const Options& o) { return !o.depthPriors.empty() || o.planePriors != 0; }
inline bool prior_sweeps_after(const Options& o, int it) { return has_priors(o) && it == o.estimationItersExternal - 2; }
inline bool priors_never_used(const Options& o) { return has_priors(o) && o.estimationItersExternal < 2; }
inline std::string export_prior_path(const Options& o, uint32_t id) { return sceneio::map_path(o.exportPriors, "/depth%04u.prior.dmap", id); }
// the parameters of the plane detection as the options give them (the rest: the library's defaults, region label 255)
inline hcmvs_plane_prior_params plane_prior_params(const Options& o, hcmvs_plane_prior_params p) {
	p.region_label = 255; p.probability = o.ransacProbability; p.epsilon_mul = o.ransacEpsilon; p.min_points_div = o.ransacMinPoints; p.seed = o.sampleSeed;
	p.cluster_mul = o.planePriors && o.planeClusters ? o.ransacCluster : 0.f; // --plane-clusters 1: --ransac-cluster is the cell edge in average spacings
	p.refit_iters = o.planePriors ? o.planeRefit : 0;                         // --plane-refit n: least-squares steps on every round's winner
	return p;
}
inline std::string prior_path(const Options& o, uint32_t id) { return sceneio::map_path(o.depthPriors, "/depth%04u.prior.dmap", id); }
// --n-filter: the filter stage hands the maps of every image that has them to the saver
inline bool stage_submits_final(const Options& o) { return o.nFilter != 0; }

} // namespace driverplan

#endif
