// city2ba (MI355X build) -- command line with the reference's subcommands and flag names
// (src/bin/city2ba.rs:113-260), written against the C ABI only (include/city2ba_hip.h), i.e. exactly
// what a Rust host would call.
//
//   city2ba synthetic OUT [--blocks N --cameras-per-block N --points-per-block N --max-dist X
//                          --camera-height X --point-height X --block-inset X --block-length X]
//   city2ba synthetic-line OUT [--cameras N --points N --max-dist X --camera-height X --point-height X
//                               --point-offset X --length X]
//   city2ba noise IN OUT [--rotation-std X --translation-std X --point-std X --observation-std X
//                         --drift-std X --drift-strength X --fixed-drift --drift-angle X
//                         --sin-strength X --sin-frequency X --mismatch-chance X --drop-features X
//                         --split-landmarks X --join-landmarks X] [--seed N] [--gpus N | --devices a,b,...]
//                        [--index-noise host|device]   (extension: with `device` the four index passes run in place on the
//                                                       resident problem, by counter-based draws: c2b_problem_drop_features, ...)
//
//   city2ba generate FILE OUT [--cameras N --intrinsics-start x,y,z --intrinsics-end x,y,z --points N --max-dist X
//                              --ground X --height X --no-lcc --move-to-origin --path NAME --step-size X] [--seed N]
//                             [--exact-lcc]   (extension: cull without the reference's observation-filter quirk at
//                                              src/baproblem.rs:523, which discards most observations whenever the
//                                              graph holds unseen points)
//   city2ba ply IN OUT
//   city2ba solve IN OUT [--iterations N --lambda X --pcg-iterations N --pcg-tol X --function-tol X --gradient-tol X
//                         --parameter-tol X --loss squared|huber|cauchy|soft-l1 --loss-scale X
//                         --preconditioner block-jacobi|schur-jacobi --schur implicit|explicit --inner-iterations N
//                         --linear-solver pcg|cholesky
//                         --fix-intrinsics --fix-first-camera
//                         --filter-max-error X --filter-rounds N --filter-in-front
//                         --prior-from FILE [--prior-center-sigma S|SX,SY,SZ] [--prior-intrinsics-sigma SF,SK1,SK2]
//                         [--prior-point-sigma S [--prior-point-every N]] [--window LO:HI [--no-halo]]
//                         [--window-around C[,C...] [--hops N] [--min-shared K] [--max-cameras M] [--no-halo]]]
//                        (extension: Levenberg-Marquardt on the device, c2b_problem_levenberg_marquardt; with
//                         --filter-max-error: N times solve + c2b_problem_filter_observations, then a solve without a loss;
//                         with --window: cameras LO .. HI-1 alone, c2b_problem_window + c2b_problem_write_back;
//                         with --window-around: the covisibility neighbourhood of the cameras given, c2b_problem_neighbourhood)
//   city2ba covisibility IN [--min-shared K]   (one line: cameras, undirected edges, maximum degree, isolated cameras of the
//                         camera covisibility graph, c2b_problem_covisibility)
//   city2ba compare EST REF [--on cameras|points|both] [--no-scale] [--max-dist D [--rounds N]] [--apply OUT]
//                        (one JSON line: the similarity that takes EST onto REF, the status and the camera and point errors that
//                         remain, c2b_problem_align; --apply: EST moved into REF's frame, c2b_problem_transform)
//   city2ba triangulate IN OUT [--min-angle DEG] [--max-error X [--min-inliers N] [--max-hypotheses H] [--drop-outliers]]
//                        (extension: the points from the cameras and observations, c2b_problem_triangulate_points; with
//                         --max-error: from the rays that agree with each other, c2b_problem_triangulate_consensus)
//   city2ba resect IN OUT [--min-points N] [--min-gap G] [--max-error X [--min-inliers N] [--max-hypotheses H] [--drop-outliers]]
//                        (extension: the camera poses from the points and observations, c2b_problem_resect_cameras; with
//                         --max-error: from the observations that agree with each other, c2b_problem_resect_consensus)
//   city2ba merge IN OUT --radius R --max-error X [--rounds N]
//                        (extension: duplicate landmarks merged, the repair of --split-landmarks, c2b_problem_merge_points;
//                         the absorbed points stay in the file as unobserved points, nothing is culled)
//   city2ba rematch IN OUT --radius R --max-error X [--min-fits N]
//                        (extension: wrong point indices put right, the repair of --mismatch-chance and --join-landmarks that
//                         keeps the observation, c2b_problem_rematch_observations; whoever fits no point is removed)
//   city2ba refine IN OUT [--cameras | --alternate N] [--rounds N] [--lambda L] [--loss KIND --loss-scale A] [--function-tol T] [--gradient-tol T]
//                         [--parameter-tol T]
//                        (extension: every point re-minimised by itself with the cameras held, per-point Levenberg-Marquardt,
//                         c2b_problem_refine_points; --cameras: every camera with the points held, c2b_problem_refine_cameras;
//                         --alternate N: N sweeps of both)
//
// `generate` casts its rays by brute force over the triangles instead of through Embree.  Every random draw is
// seeded (--seed; default: std::random_device) where the reference uses thread_rng().
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <random>
#include <stdexcept>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/city2ba_hip.h"
#include "../../include/city2ba_hip_host.h"
#include "../../include/city2ba_hip_experimental.h"

namespace {

// Leaves at once: std::exit would run static destructors (the HIP runtime's among them) while a helper thread -- the
// mesh loader, the hierarchy builder of run_generate -- may still be running.
[[noreturn]] void die(const std::string &msg) {
    std::fflush(stdout);
    std::fprintf(stderr, "Error: %s\n", msg.c_str());
    std::fflush(stderr);
    std::_Exit(1);
}

void ck(int rc) {
    if (rc != C2B_OK) die(c2b_last_error());
}

// Rust `{:.2e}`: "1.23e-5", "0.00e0"
std::string sci2(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    if (v == 0.0) return "0.00e0";
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.2e", v);
    std::string s(buf);
    const size_t e = s.find('e');
    const int ex = std::atoi(s.c_str() + e + 1);
    return s.substr(0, e) + "e" + std::to_string(ex);
}

struct Args {
    std::vector<std::string> positional;
    std::map<std::string, std::string> opt;
    bool has(const std::string &k) const { return opt.count(k) != 0; }
    double f(const std::string &k, double dflt) const {
        auto it = opt.find(k);
        if (it == opt.end()) return dflt;
        char *end = nullptr;
        const double v = std::strtod(it->second.c_str(), &end);
        if (end == it->second.c_str() || *end) die("Invalid value for '--" + k + " <" + k + ">': invalid float literal");
        return v;
    }
    int64_t i(const std::string &k, int64_t dflt) const {
        auto it = opt.find(k);
        if (it == opt.end()) return dflt;
        char *end = nullptr;
        const long long v = std::strtoll(it->second.c_str(), &end, 10);
        if (end == it->second.c_str() || *end || v < 0) die("Invalid value for '--" + k + " <" + k + ">': invalid digit found in string");
        return (int64_t)v;
    }
};

Args parse(int argc, char **argv, int first, const std::vector<std::string> &flags, const std::vector<std::string> &values) {
    Args a;
    for (int k = first; k < argc; ++k) {
        std::string s = argv[k];
        if (s.rfind("--", 0) == 0) {
            std::string key = s.substr(2), val;
            const size_t eq = key.find('=');
            bool has_val = false;
            if (eq != std::string::npos) { val = key.substr(eq + 1); key = key.substr(0, eq); has_val = true; }
            bool is_flag = false, is_value = false;
            for (auto &f : flags) if (f == key) is_flag = true;
            for (auto &v : values) if (v == key) is_value = true;
            if (is_flag) { a.opt[key] = "1"; continue; }
            if (!is_value) die("Found argument '--" + key + "' which wasn't expected, or isn't valid in this context");
            if (!has_val) {
                if (k + 1 >= argc) die("The argument '--" + key + " <" + key + ">' requires a value but none was supplied");
                val = argv[++k];
            }
            a.opt[key] = val;
        } else {
            a.positional.push_back(s);
        }
    }
    return a;
}

// "a,b,c" -> its tokens, empty ones included ("" is one empty token); what a token must be is the caller's to check
std::vector<std::string> split_commas(const std::string &s) {
    std::vector<std::string> tok;
    for (size_t pos = 0; pos <= s.size();) {
        const size_t comma = std::min(s.find(',', pos), s.size());
        tok.push_back(s.substr(pos, comma - pos));
        pos = comma + 1;
    }
    return tok;
}

// --seed, or the reference's unseeded thread_rng()
uint64_t seed_of(const Args &a) {
    if (a.has("seed")) return (uint64_t)a.i("seed", 0);
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ rd();
}

// The library takes its behaviour switches as c2b_problem_options, not from the environment; this program -- a caller of
// the C ABI like any other -- keeps its environment variables (README.md) and turns them into those options for every
// problem it makes.
static int env_int(const char *name, int dflt) { const char *v = std::getenv(name); return v && *v ? std::atoi(v) : dflt; }
static bool env_on(const char *name) { const char *v = std::getenv(name); return v && *v && std::strcmp(v, "0") != 0; }
static int create_problem(int device, c2b_problem **out) {
    const int rc = c2b_problem_create(device, out);
    if (rc) return rc;
    c2b_problem_options o;
    c2b_problem_options_init(&o);
    o.host_text = env_on("C2B_HOST_TEXT");
    o.text_device_strict = env_on("C2B_TEXT_DEVICE_STRICT");
    o.read_threads = std::max(0, std::min(64, env_int("C2B_READ_THREADS", 0)));
    o.io_threads = std::max(0, std::min(64, env_int("C2B_IO_THREADS", 0)));
    o.rank_sort_max_row = std::max(0, env_int("C2B_RANK_SORT_MAX_ROW", 0));
    if (const char *v = std::getenv("C2B_TEXT_DEVICE_MIN_BYTES")) o.text_device_min_bytes = (int64_t)std::strtoll(v, nullptr, 10);
    return c2b_problem_set_options(*out, &o);
}

// C2B_TIMING=1: wall time of each phase on stderr
struct PhaseTimer {
    bool on = std::getenv("C2B_TIMING") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void mark(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[timing] %-50s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
};

struct HostProblem {
    int64_t n_cam = 0, n_pts = 0, n_obs = 0;
    std::vector<double> cams15, pts, uv;                                  // each with one spare element, so that data() is never null
    std::vector<uint64_t> row_ptr, pt_idx;
};

// the resident problem (cameras as in-memory records, points, graph, observations) on the host
void download_problem(c2b_problem *p, HostProblem &hp) {
    ck(c2b_problem_sizes(p, &hp.n_cam, &hp.n_pts, &hp.n_obs));
    hp.cams15.assign((size_t)hp.n_cam * 15 + 1, 0.0);
    hp.pts.assign((size_t)hp.n_pts * 3 + 1, 0.0);
    hp.uv.assign((size_t)hp.n_obs * 2 + 1, 0.0);
    hp.row_ptr.assign((size_t)hp.n_cam + 1, 0);
    hp.pt_idx.assign((size_t)hp.n_obs + 1, 0);
    ck(c2b_problem_download(p, hp.cams15.data(), hp.pts.data(), hp.uv.data()));
    ck(c2b_problem_download_graph(p, hp.row_ptr.data(), hp.pt_idx.data()));
}

// the report lines: BAProblem's Display, and run_noise's three (src/bin/city2ba.rs:283-287, :342-354)
void print_problem(int64_t n_cam, int64_t n_pts, int64_t n_obs) {
    std::printf("Bundle Adjustment Problem with %lld cameras, %lld points, and %lld observations\n", (long long)n_cam, (long long)n_pts, (long long)n_obs);
}
void print_initial_error(double l1, double l2) { std::printf("Initial error: %s (L1) %s (L2)\n", sci2(l1).c_str(), sci2(l2).c_str()); }
void print_correspondences(int64_t n_cam, int64_t n_pts, int64_t n_obs) {
    std::printf("BA Problem with %lld cameras, %lld points, %lld correspondences\n", (long long)n_cam, (long long)n_pts, (long long)n_obs);
}
void print_final_error(double l1, double l2) { std::printf("Final error: %s (L1) %s (L2)\n", sci2(l1).c_str(), sci2(l2).c_str()); }

// A problem on `device` decoded from `file` there; and its end: written to `file` from the device, destroyed.
c2b_problem *read_problem(PhaseTimer &timer, int device, const std::string &file) {
    c2b_problem *p = nullptr;
    ck(create_problem(device, &p));
    timer.mark("problem_create (HIP runtime start)");
    ck(c2b_problem_read(p, file.c_str(), -1));
    timer.mark("read (c2b_problem_read: decoded on the device)");
    return p;
}

void close_problem(PhaseTimer &timer, c2b_problem *p, const std::string &file) {
    ck(c2b_problem_write(p, file.c_str(), -1));
    timer.mark("write (c2b_problem_write: the file image is built on the device)");
    c2b_problem_destroy(p);
}

// synthetic_grid / synthetic_line (src/synthetic.rs:163-300, :313-381) and the tail of their subcommands
// (src/bin/city2ba.rs:447-478), everything on the resident problem: the layout loops, the visibility loop -- candidates
// within max_dist, hits_building, the predicate --, cull, the Display line, and the file image.  Only the file's bytes
// leave the device.  C2B_HOST_CANDIDATES=1 takes rounds 1-3's route (layout and candidate search on the host, 47.5 M
// pairs uploaded at --blocks 128, the arrays downloaded and serialised by the host) for comparison; same file.
struct Layout {
    bool grid = true;
    int64_t cpb = 0, ppb = 0, blocks = 0, n_cam = 0, n_pts = 0;              // grid: per block; line: totals in n_cam / n_pts
    double L = 0, inset = 0, cam_h = 0, pt_h = 0, length = 0, point_offset = 0;
};

int generate_cull_write(const Args &a, const Layout &lay) {
    PhaseTimer timer;
    c2b_problem *p = nullptr;
    ck(create_problem((int)a.i("device", 0), &p));
    timer.mark("problem_create (HIP runtime start)");
    const double max_dist = a.f("max-dist", 10);
    const std::string &out = a.positional[0];
    const bool host_route = std::getenv("C2B_HOST_CANDIDATES") != nullptr;
    const bool occlusion = lay.grid;
    const double L = lay.grid ? lay.L : 1.0, inset = lay.grid ? lay.inset : 0.0;
    if (host_route) {
        int64_t n_cam = lay.n_cam, n_pts = lay.n_pts;
        if (lay.grid) ck(c2b_synthetic_grid_sizes(lay.cpb, lay.ppb, lay.blocks, &n_cam, &n_pts));
        std::vector<double> pos((size_t)n_cam * 3), dir((size_t)n_cam * 9), pts((size_t)n_pts * 3), cams15((size_t)n_cam * 15);
        if (lay.grid) ck(c2b_synthetic_grid_layout(lay.cpb, lay.ppb, lay.blocks, lay.L, lay.inset, lay.cam_h, lay.pt_h, pos.data(), dir.data(), pts.data()));
        else ck(c2b_synthetic_line_layout(n_cam, n_pts, lay.length, lay.point_offset, lay.cam_h, lay.pt_h, pos.data(), dir.data(), pts.data()));
        ck(c2b_problem_from_position_direction(p, n_cam, pos.data(), dir.data(), cams15.data()));
        std::vector<uint64_t> empty_rows((size_t)n_cam + 1, 0);
        ck(c2b_problem_upload(p, n_cam, cams15.data(), n_pts, pts.data(), empty_rows.data(), nullptr, nullptr));
        timer.mark("layout (host) + from_position_direction + upload");
        std::vector<double> centers((size_t)n_cam * 3);
        ck(c2b_problem_centers(p, centers.data()));
        c2b_pairs *pairs = nullptr;
        const int threads = (int)std::max(1u, std::thread::hardware_concurrency());
        ck(c2b_candidate_pairs(centers.data(), n_cam, pts.data(), n_pts, max_dist, 0, n_cam, occlusion ? 1 : 0, L, inset, threads, &pairs));
        timer.mark("centres + candidate pairs (host, threaded)");
        std::vector<uint64_t> rows((size_t)n_cam + 1, 0);
        ck(c2b_problem_visibility_pairs_compact(p, c2b_pairs_count(pairs), c2b_pairs_cam_idx(pairs), c2b_pairs_pt_idx(pairs), max_dist, rows.data()));
        c2b_pairs_free(pairs);
        timer.mark("visibility predicate + compaction (device)");
    } else {
        if (lay.grid) ck(c2b_problem_synthetic_grid_layout(p, lay.cpb, lay.ppb, lay.blocks, lay.L, lay.inset, lay.cam_h, lay.pt_h));
        else ck(c2b_problem_synthetic_line_layout(p, lay.n_cam, lay.n_pts, lay.length, lay.point_offset, lay.cam_h, lay.pt_h));
        timer.mark("layout (device)");
        ck(c2b_problem_visibility_within_distance(p, max_dist, occlusion ? 1 : 0, L, inset, nullptr));
        timer.mark("candidates + hits_building + predicate (device)");
    }
    ck(c2b_problem_adopt_visibility(p));
    // .cull(), src/synthetic.rs:299 -- on the device
    ck(c2b_problem_cull(p, 1));
    timer.mark("adopt + cull (device)");
    if (host_route) {
        HostProblem hp;
        download_problem(p, hp);
        timer.mark("download");
        print_problem(hp.n_cam, hp.n_pts, hp.n_obs);
        std::vector<double> bal9((size_t)hp.n_cam * 9);
        ck(c2b_problem_download_bal(p, bal9.data()));
        timer.mark("to_vec + download");
        ck(c2b_bal_write(out.c_str(), hp.n_cam, bal9.data(), hp.n_pts, hp.pts.data(), hp.row_ptr.data(), hp.pt_idx.data(), hp.uv.data()));
        timer.mark("write");
        c2b_problem_destroy(p);
    } else {
        int64_t nc = 0, np = 0, no = 0;
        ck(c2b_problem_sizes(p, &nc, &np, &no));
        print_problem(nc, np, no);
        close_problem(timer, p, out);
    }
    return 0;
}

int run_synthetic(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"cameras-per-block", "points-per-block", "max-dist", "camera-height",
                                             "point-height", "block-inset", "block-length", "blocks", "device"});
    if (a.positional.size() != 1) die("The following required arguments were not provided:\n    <OUTPUT>");
    Layout lay;
    lay.cpb = a.i("cameras-per-block", 10); lay.ppb = a.i("points-per-block", 10); lay.blocks = a.i("blocks", 5);
    lay.cam_h = a.f("camera-height", 1); lay.pt_h = a.f("point-height", 1);
    lay.inset = a.f("block-inset", 1); lay.L = a.f("block-length", 20);
    return generate_cull_write(a, lay);
}

int run_synthetic_line(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"cameras", "points", "max-dist", "camera-height", "point-height",
                                             "point-offset", "length", "device"});
    if (a.positional.size() != 1) die("The following required arguments were not provided:\n    <OUTPUT>");
    Layout lay;
    lay.grid = false;
    lay.n_cam = a.i("cameras", 10); lay.n_pts = a.i("points", 10);
    lay.length = a.f("length", 20); lay.point_offset = a.f("point-offset", 1);
    lay.cam_h = a.f("camera-height", 1); lay.pt_h = a.f("point-height", 1);
    return generate_cull_write(a, lay);
}

// Every option of `noise`, converted before a device exists or the input is opened; a worker thread sees only this.  (Not
// looked at, as no route reads it: --sin-frequency without --sin-strength, --gpus beside --devices, --device when sharded.)
struct NoiseOptions {
    uint64_t seed = 0;
    double drop = 1, join = 0, split = 0, mismatch = 0, drift_strength = 0, drift_angle = 0, drift_std = 0, sin_strength = 0, sin_frequency = 1;
    double translation_std = 0, rotation_std = 0, point_std = 0, observation_std = 0;
    bool fixed_drift = false;
    int device = 0;                // the GPU of the unsharded routes
    std::vector<int> devices;      // --gpus N / --devices a,b,...: the sharded route when not empty
    bool index_on_device = false;  // --index-noise device: the index passes in place on the resident problem (another draw scheme)
    bool reshapes() const { return drop < 1.0 || join > 0.0 || split > 0.0; }
};

NoiseOptions noise_options(const Args &a) {
    NoiseOptions o;
    o.seed = seed_of(a);
    o.drop = a.f("drop-features", 1.0); o.join = a.f("join-landmarks", 0.0); o.split = a.f("split-landmarks", 0.0);
    o.mismatch = a.f("mismatch-chance", 0.0);
    o.fixed_drift = a.has("fixed-drift");
    o.drift_strength = a.f("drift-strength", 0); o.drift_angle = a.f("drift-angle", 0); o.drift_std = a.f("drift-std", 0);
    o.sin_strength = a.f("sin-strength", 0);
    if (o.sin_strength > 0.0) o.sin_frequency = a.f("sin-frequency", 1);
    o.translation_std = a.f("translation-std", 0); o.rotation_std = a.f("rotation-std", 0);
    o.point_std = a.f("point-std", 0); o.observation_std = a.f("observation-std", 0);
    if (a.has("index-noise")) {
        const std::string &v = a.opt.at("index-noise");
        if (v != "host" && v != "device") die("Invalid value for '--index-noise <index-noise>': expected host or device");
        o.index_on_device = v == "device";
        if (o.index_on_device && (a.has("gpus") || a.has("devices")))
            die("--index-noise device runs on one GPU: it cannot be combined with --gpus or --devices (the index passes are not sharded)");
    }
    if (!a.has("devices") && !a.has("gpus")) {
        o.device = (int)a.i("device", 0);
        return o;
    }
    if (!a.has("devices"))
        for (int64_t k = 0; k < a.i("gpus", 1); ++k) o.devices.push_back((int)k);
    else
        for (const std::string &tok : split_commas(a.opt.at("devices"))) {
            char *end = nullptr;
            const long v = std::strtol(tok.c_str(), &end, 10);
            if (tok.empty() || *end || v < 0) die("Invalid value for '--devices <devices>': expected a,b,c");
            o.devices.push_back((int)v);
        }
    if (o.devices.size() < 1 || o.devices.size() > 64) die("Invalid value for '--gpus <gpus>': expected 1..64");
    return o;
}

// A problem on the host as a .bal holds it: cameras as 9-vectors, points, the camera-major observation list.
struct HostBal {
    int64_t n_cam = 0, n_pts = 0, n_obs = 0;
    size_t pts_cap = 0;            // points `pts` has room for: split_landmarks appends
    std::vector<double> bal9, pts, uv;
    std::vector<uint64_t> row_ptr, pt_idx;
};

HostBal read_bal(const std::string &path, double split = 0.0) {
    HostBal h;
    c2b_balfile *f = nullptr;
    ck(c2b_bal_read(path.c_str(), &f));
    ck(c2b_bal_sizes(f, &h.n_cam, &h.n_pts, &h.n_obs));
    h.pts_cap = (size_t)h.n_pts + (split > 0.0 ? (size_t)(std::min(split, 1.0) * (double)h.n_pts) + 1 : 0);
    h.bal9.resize((size_t)h.n_cam * 9 + 1); h.pts.resize(h.pts_cap * 3 + 1); h.uv.resize((size_t)h.n_obs * 2 + 1);
    h.row_ptr.resize((size_t)h.n_cam + 1); h.pt_idx.resize((size_t)h.n_obs + 1);
    ck(c2b_bal_copy(f, h.bal9.data(), h.pts.data(), h.row_ptr.data(), h.pt_idx.data(), h.uv.data()));
    c2b_bal_close(f);
    return h;
}

int upload_bal(c2b_problem *p, const HostBal &h) {
    return c2b_problem_upload_bal(p, h.n_cam, h.bal9.data(), h.n_pts, h.pts.data(), h.row_ptr.data(), h.pt_idx.data(), h.uv.data());
}
void write_bal(const std::string &path, const HostBal &h) {
    ck(c2b_bal_write(path.c_str(), h.n_cam, h.bal9.data(), h.n_pts, h.pts.data(), h.row_ptr.data(), h.pt_idx.data(), h.uv.data()));
}

// The index-corruption passes on the host arrays, each followed by cull() (src/bin/city2ba.rs:288-303); camera rows stay
// 9-vectors (cull treats them as opaque).  Returns whether anything was reshaped.
bool reshape(HostBal &h, const NoiseOptions &o) {
    bool reshaped = false;
    auto cull = [&]() {
        ck(c2b_cull(&h.n_cam, h.bal9.data(), 9, &h.n_pts, h.pts.data(), h.row_ptr.data(), h.pt_idx.data(), h.uv.data(), 1));
        h.n_obs = (int64_t)h.row_ptr[(size_t)h.n_cam];
        reshaped = true;
    };
    if (o.drop < 1.0) {
        ck(c2b_drop_features(h.n_cam, h.row_ptr.data(), h.pt_idx.data(), h.uv.data(), o.drop, o.seed + 2));
        cull();
    }
    if (o.join > 0.0) {
        // the reference passes opt.split_landmarks as the fraction here (src/bin/city2ba.rs:296)
        ck(c2b_join_landmarks(h.n_pts, h.pts.data(), (int64_t)h.row_ptr[(size_t)h.n_cam], h.pt_idx.data(), o.split, o.seed + 3));
        cull();
    }
    if (o.split > 0.0) {
        ck(c2b_split_landmarks(&h.n_pts, h.pts.data(), (int64_t)h.pts_cap, (int64_t)h.row_ptr[(size_t)h.n_cam], h.pt_idx.data(), o.split, o.seed + 4));
        cull();
    }
    // (the sharded route refuses an empty input here as well: there is nothing to cut into ranges)
    if ((reshaped || !o.devices.empty()) && (h.n_cam == 0 || h.n_pts == 0)) die("EmptyProblem: nothing remains after culling");
    return reshaped;
}

// add_incorrect_correspondences on the host arrays (src/bin/city2ba.rs:341)
void scramble(HostBal &h, const NoiseOptions &o) {
    ck(c2b_add_incorrect_correspondences(h.n_cam, h.row_ptr.data(), h.pt_idx.data(), h.uv.data(), o.mismatch, o.seed + 5));
}

// The arithmetic chain of run_noise on one problem (comm == nullptr) or on one shard of it (the collective *_sharded
// entries).  Returns the first failing call's status and never dies: shard workers call it.
int perturb(c2b_problem *p, c2b_comm *comm, const NoiseOptions &o, double *l1, double *l2) {
    int rc = C2B_OK;
    double stats[C2B_STATS_DOUBLES];
    const double *dir = nullptr;                                         // src/bin/city2ba.rs:305-316: drift is ALWAYS applied, even with zero strength
    if (o.fixed_drift) {
        if ((rc = comm ? c2b_problem_stats_sharded(p, comm, stats) : c2b_problem_stats(p, stats))) return rc;
        dir = stats + 3;
    }
    if (comm) rc = c2b_problem_add_drift_sharded(p, comm, o.drift_strength, o.drift_angle, o.drift_std, dir, o.seed);
    else if (dir) rc = c2b_problem_add_drift(p, o.drift_strength, o.drift_angle, o.drift_std, dir, o.seed);
    else rc = c2b_problem_add_drift_normalized(p, o.drift_strength, o.drift_angle, o.drift_std, o.seed);
    if (rc) return rc;
    if (o.sin_strength > 0.0) {                                          // :318-333
        const double dx[3] = {1, 0, 0}, dz[3] = {0, 0, 1}, up[3] = {0, 1, 0};
        for (const double *d : {dx, dz}) {
            rc = comm ? c2b_problem_add_sin_noise_sharded(p, comm, d, up, o.sin_strength, o.sin_frequency)
                      : c2b_problem_add_sin_noise(p, d, up, o.sin_strength, o.sin_frequency);
            if (rc) return rc;
        }
    }
    // :334-340 (always) fused with the final errors of :350-354: the observation pass draws, perturbs, stores, projects
    // and folds both norms in one launch (per shard).  With --mismatch-chance the errors are evaluated again after the scramble.
    return comm ? c2b_problem_add_noise_errors_l1_l2_sharded(p, comm, o.translation_std, o.rotation_std, o.point_std, o.observation_std, o.seed + 1, l1, l2)
                : c2b_problem_add_noise_errors_l1_l2(p, o.translation_std, o.rotation_std, o.point_std, o.observation_std, o.seed + 1, l1, l2);
}

// `noise --gpus N` (or --devices a,b,...): run_noise (src/bin/city2ba.rs:280-357) with the problem sharded over N GPUs of
// this node, driven from ONE process -- SURVEY 8(b)'s ctx_create(n_dev, dev_ids).  The index-corruption passes and their
// culls run on the host arrays as in the single-GPU path; then cameras are cut into N contiguous ranges holding equal
// numbers of observations (c2b_partition_cameras), every GPU gets its range, that range's observations and ALL points
// (one c2b_problem each, marked with c2b_problem_set_shard), and one host thread per GPU runs the same sequence of
// collective Level-1 calls (c2b_problem_*_sharded: statistics and errors go through RCCL, c2b_comm_init_all).  Draws
// are keyed by global indices, so the written file is the same for every N up to rounding: the statistics that scale
// the perturbations (mean, std) are sums of per-rank shares, whose last bits depend on how the cameras were cut.
// On return `h` holds the noised problem; the caller writes it.
void run_noise_sharded(const NoiseOptions &o, HostBal &h) {
    const std::vector<int> &devs = o.devices;
    const int N = (int)devs.size();
    int visible = 0;
    ck(c2b_device_count(&visible));
    for (int d : devs) if (d >= visible) die("--gpus / --devices: device " + std::to_string(d) + " is not visible (" + std::to_string(visible) + " devices)");

    std::vector<c2b_comm *> comms((size_t)N, nullptr);
    ck(c2b_comm_init_all(N, devs.data(), comms.data()));
    double err[4] = {0, 0, 0, 0};                                         // initial L1, L2, final L1, L2 (written by rank 0)
    std::vector<double> pts_out;

    // One pass over the GPUs: cut the cameras, give every GPU its shard, run the collective sequence on one host thread
    // per GPU.  with_initial: evaluate the error of the problem as uploaded; with_noise: drift, sine, Gaussian noise, final
    // error, download.
    auto pass = [&](bool with_initial, bool with_noise) {
        std::vector<int64_t> bounds((size_t)N + 1);
        ck(c2b_partition_cameras(h.row_ptr.data(), h.n_cam, N, bounds.data()));
        int nonempty = 0;
        for (int k = 0; k < N; ++k) nonempty += bounds[(size_t)k + 1] > bounds[(size_t)k];
        if (nonempty < N)
            die("--gpus " + std::to_string(N) + ": the problem's " + std::to_string(h.n_cam) + " cameras (" + std::to_string(h.n_obs) +
                " observations) cut into only " + std::to_string(nonempty) + " non-empty ranges; use --gpus " + std::to_string(std::max(1, nonempty)));
        std::vector<std::string> failures((size_t)N);
        if (with_noise) {
            std::fprintf(stderr, "noise on %d GPU%s through %s; observations per GPU:", N, N == 1 ? "" : "s", c2b_comm_backend());
            for (int k = 0; k < N; ++k)
                std::fprintf(stderr, " %llu", (unsigned long long)(h.row_ptr[(size_t)bounds[(size_t)k + 1]] - h.row_ptr[(size_t)bounds[(size_t)k]]));
            std::fprintf(stderr, "\n");
            pts_out.assign((size_t)h.n_pts * 3 + 1, 0.0);
        }
        std::vector<std::thread> workers;
        for (int k = 0; k < N; ++k) {
            workers.emplace_back([&, k]() {
                // a failing call ends THIS worker with its message (reported after the join; std::exit from a worker thread
                // would run static destructors under the other workers' feet).  A rank that fails between two collectives
                // leaves its peers waiting in the next one -- the same as a rank of an MPI job dying
                auto ck = [&](int rc) { if (rc != C2B_OK) throw std::runtime_error(c2b_last_error()); };
                try {
                const int64_t lo = bounds[(size_t)k], hi = bounds[(size_t)k + 1], nc = hi - lo;
                const uint64_t o0 = h.row_ptr[(size_t)lo];
                std::vector<uint64_t> rp((size_t)nc + 1);
                for (int64_t c = 0; c <= nc; ++c) rp[(size_t)c] = h.row_ptr[(size_t)(lo + c)] - o0;
                c2b_problem *p = nullptr;
                ck(create_problem(devs[(size_t)k], &p));
                ck(c2b_problem_upload_bal(p, nc, h.bal9.data() + 9 * lo, h.n_pts, h.pts.data(), rp.data(), h.pt_idx.data() + o0, h.uv.data() + 2 * o0));
                ck(c2b_problem_set_shard(p, lo, h.n_cam, (int64_t)o0));
                c2b_comm *comm = comms[(size_t)k];
                double l1, l2;
                if (with_initial) {           // both norms from one pass, ONE 2-element all-reduce (src/bin/city2ba.rs:283-287)
                    ck(c2b_problem_total_reprojection_errors_l1_l2_sharded(p, comm, &l1, &l2));
                    if (k == 0) { err[0] = l1; err[1] = l2; }
                }
                if (with_noise) {
                    ck(perturb(p, comm, o, &l1, &l2));
                    if (k == 0) { err[2] = l1; err[3] = l2; }
                    // every shard's cameras and observations go back to their rows of the host arrays; the points
                    // (identical on every GPU) come from rank 0
                    ck(c2b_problem_download(p, nullptr, k == 0 ? pts_out.data() : nullptr, h.uv.data() + 2 * o0));
                    ck(c2b_problem_download_bal(p, h.bal9.data() + 9 * lo));
                }
                c2b_problem_destroy(p);
                } catch (const std::exception &e) { failures[(size_t)k] = e.what(); }
            });
        }
        for (auto &w : workers) w.join();
        for (int k = 0; k < N; ++k)
            if (!failures[(size_t)k].empty()) die("GPU " + std::to_string(devs[(size_t)k]) + " (rank " + std::to_string(k) + "): " + failures[(size_t)k]);
    };

    // host-side index corruption + cull, exactly as in the single-GPU path (src/bin/city2ba.rs:288-303): the reference
    // prints the initial error BEFORE these passes, so when any of them is requested the problem visits the GPUs twice
    if (o.reshapes()) pass(true, false);
    reshape(h, o);
    pass(!o.reshapes(), true);
    for (c2b_comm *c : comms) c2b_comm_destroy(c);
    std::copy(pts_out.begin(), pts_out.begin() + (size_t)h.n_pts * 3, h.pts.begin());
    print_initial_error(err[0], err[1]);
    if (o.mismatch > 0.0) scramble(h, o);                                // :341, on the noised image positions (host arrays)
    print_correspondences(h.n_cam, h.n_pts, h.n_obs);
    if (o.mismatch > 0.0) {
        // the reference reports the error AFTER the correspondences were scrambled: one more sharded pass would need a
        // re-upload; the single-GPU evaluation of the final arrays gives the same number
        c2b_problem *p = nullptr;
        ck(create_problem(devs[0], &p));
        ck(upload_bal(p, h));
        ck(c2b_problem_total_reprojection_errors_l1_l2(p, &err[2], &err[3]));
        c2b_problem_destroy(p);
    }
    print_final_error(err[2], err[3]);
}

int run_noise(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"fixed-drift"},
                         {"rotation-std", "translation-std", "point-std", "observation-std", "drift-std", "drift-strength",
                          "drift-angle", "mismatch-chance", "drop-features", "split-landmarks", "join-landmarks",
                          "sin-strength", "sin-frequency", "seed", "device", "gpus", "devices", "index-noise"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    const NoiseOptions o = noise_options(a);                             // every value is converted before the device is touched
    const std::string &in = a.positional[0], &out = a.positional[1];
    double l1, l2;

    // The common case -- no index-corruption pass (src/bin/city2ba.rs:288-303, :341), one GPU -- never leaves the device:
    // the file is decoded into the resident problem (c2b_problem_read), the whole chain of src/bin/city2ba.rs:280-357 runs
    // on it, and the output file's image is assembled there (c2b_problem_write).  Both error pairs cost one pass each, the
    // second one fused with add_noise's observation pass.
    if (!o.reshapes() && !(o.mismatch > 0.0) && o.devices.empty() && !std::getenv("C2B_HOST_IO")) {
        PhaseTimer timer;
        c2b_problem *p = read_problem(timer, o.device, in);
        ck(c2b_problem_total_reprojection_errors_l1_l2(p, &l1, &l2));
        print_initial_error(l1, l2);
        ck(perturb(p, nullptr, o, &l1, &l2));
        int64_t nc = 0, np = 0, no = 0;
        ck(c2b_problem_sizes(p, &nc, &np, &no));
        print_correspondences(nc, np, no);
        print_final_error(l1, l2);
        timer.mark("errors + drift + noise (device)");
        close_problem(timer, p, out);
        return 0;
    }

    // --index-noise device: the same chain in the reference's order (src/bin/city2ba.rs:288-303, :341) with the four index
    // passes in place on the resident problem -- the problem is read on the device and never comes down.
    if (o.index_on_device) {
        PhaseTimer timer;
        c2b_problem *p = read_problem(timer, o.device, in);
        ck(c2b_problem_total_reprojection_errors_l1_l2(p, &l1, &l2));
        print_initial_error(l1, l2);
        timer.mark("initial errors (device)");
        if (o.drop < 1.0) {
            ck(c2b_problem_drop_features(p, o.drop, o.seed + 2, nullptr));
            ck(c2b_problem_cull(p, 1));
            timer.mark("drop_features + cull (device)");
        }
        if (o.join > 0.0) {                                              // the split fraction: the reference's quirk at :296
            ck(c2b_problem_join_landmarks(p, o.split, o.seed + 3, nullptr));
            ck(c2b_problem_cull(p, 1));
            timer.mark("join_landmarks + cull (device)");
        }
        if (o.split > 0.0) {
            ck(c2b_problem_split_landmarks(p, o.split, o.seed + 4, nullptr));
            ck(c2b_problem_cull(p, 1));
            timer.mark("split_landmarks + cull (device)");
        }
        int64_t nc = 0, np = 0, no = 0;
        ck(c2b_problem_sizes(p, &nc, &np, &no));
        if (o.reshapes() && (nc == 0 || np == 0)) die("EmptyProblem: nothing remains after culling");
        ck(perturb(p, nullptr, o, &l1, &l2));
        timer.mark("drift + noise + errors (device)");
        if (o.mismatch > 0.0) {                                          // :341, on the noised image positions
            ck(c2b_problem_add_incorrect_correspondences(p, o.mismatch, o.seed + 5, nullptr));
            ck(c2b_problem_total_reprojection_errors_l1_l2(p, &l1, &l2));
            timer.mark("add_incorrect_correspondences + errors (device)");
        }
        print_correspondences(nc, np, no);
        print_final_error(l1, l2);
        close_problem(timer, p, out);
        return 0;
    }

    HostBal h = read_bal(in, o.split);
    if (!o.devices.empty()) {
        run_noise_sharded(o, h);
        write_bal(out, h);
        return 0;
    }

    c2b_problem *p = nullptr;
    ck(create_problem(o.device, &p));
    ck(upload_bal(p, h));
    ck(c2b_problem_total_reprojection_errors_l1_l2(p, &l1, &l2));        // src/bin/city2ba.rs:283-287: both norms, one pass
    print_initial_error(l1, l2);
    if (reshape(h, o)) ck(upload_bal(p, h));
    ck(perturb(p, nullptr, o, &l1, &l2));
    ck(c2b_problem_download(p, nullptr, h.pts.data(), h.uv.data()));
    if (o.mismatch > 0.0) {                                              // :341, on the noised image positions
        std::vector<double> cams15((size_t)h.n_cam * 15 + 1);
        ck(c2b_problem_download(p, cams15.data(), nullptr, nullptr));
        scramble(h, o);
        ck(c2b_problem_upload(p, h.n_cam, cams15.data(), h.n_pts, h.pts.data(), h.row_ptr.data(), h.pt_idx.data(), h.uv.data()));
        ck(c2b_problem_total_reprojection_errors_l1_l2(p, &l1, &l2));
    }
    print_correspondences(h.n_cam, h.n_pts, h.n_obs);
    print_final_error(l1, l2);
    ck(c2b_problem_download_bal(p, h.bal9.data()));
    write_bal(out, h);
    c2b_problem_destroy(p);
    return 0;
}

// parse_vec3, src/bin/city2ba.rs:20-31: "x,y,z"
void parse_vec3(const Args &a, const std::string &k, double out[3]) {
    auto it = a.opt.find(k);
    if (it == a.opt.end()) return;
    const std::vector<std::string> tok = split_commas(it->second);
    for (size_t c = 0; c < 3; ++c) {                                     // a missing comma is met before the number in front of it
        if (c < 2 && tok.size() < c + 2) die("Invalid value for '--" + k + " <" + k + ">': expected x,y,z");
        char *end = nullptr;
        out[c] = std::strtod(tok[c].c_str(), &end);
        if (end == tok[c].c_str() || *end || (c == 2 && tok.size() > 3)) die("Invalid value for '--" + k + " <" + k + ">': invalid float literal");
    }
}

// Rust `{}` of an f64: shortest digits that round-trip, never scientific
std::string display_f64(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

// run_generate, src/bin/city2ba.rs:480-573.  Ray casts: brute force over the mesh's triangles (host for camera
// placement, the device occlusion kernel for the visibility graph) in place of Embree.
int run_generate(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"no-lcc", "move-to-origin", "exact-lcc"},
                         {"cameras", "intrinsics-start", "intrinsics-end", "points", "max-dist", "ground", "height", "path",
                          "step-size", "seed", "device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    if (a.has("path") && a.has("ground")) die("The argument '--path <path>' cannot be used with '--ground <ground>'");
    const int64_t num_cameras = a.i("cameras", 100), num_points = a.i("points", 1000);
    const double max_dist = a.f("max-dist", 100), ground = a.f("ground", 0), height = a.f("height", 1);
    const double step_size = a.f("step-size", 0);
    double istart[3] = {1, 0, 0}, iend[3] = {1, 0, 0};
    parse_vec3(a, "intrinsics-start", istart);
    parse_vec3(a, "intrinsics-end", iend);
    const uint64_t seed = seed_of(a);

    PhaseTimer timer;
    // Everything that needs only the file runs on a second thread while this one starts the HIP runtime (c2b_problem_create:
    // 60-260 ms that need nothing from the file) and then works on the cameras: load the mesh, find the path, move to
    // the origin, extract the triangles -- "mesh ready" -- and, when the cameras follow a path, go straight on to the
    // hierarchy of the occlusion rays (c2b_bvh_build, itself multi-threaded), which is not needed before the points are
    // sampled and the candidates found.  (Poisson placement builds the hierarchy of its downward rays itself, beside its
    // darts; the one for the occlusion rays is then started after the placement, on the same thread object.)  The
    // worker's status and message come back through `mesh`.
    struct Mesh {
        std::mutex mu;
        std::condition_variable cv;
        int stage = 0;                                        // 1: obj / path_model / tri are ready; 2: bvh too (or failed)
        int rc = C2B_OK;
        std::string err;
        c2b_obj *obj = nullptr;
        int64_t path_model = -1, n_tri = 0;
        std::vector<float> tri;
        c2b_bvh *bvh = nullptr;
        bool want_bvh = false;
        void fail_with(const std::string &m) { std::lock_guard<std::mutex> lk(mu); rc = -1; err = m; stage = 2; cv.notify_all(); }
        void reach(int s) { std::lock_guard<std::mutex> lk(mu); stage = s; cv.notify_all(); }
        void wait_for(int s) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stage >= s; }); }
    } mesh;
    auto build_bvh = [&]() {
        if (c2b_bvh_build(mesh.tri.data(), mesh.n_tri, &mesh.bvh) != C2B_OK) mesh.fail_with(c2b_last_error());
        else mesh.reach(2);
    };
    std::thread worker([&]() {
        if (c2b_obj_load(a.positional[0].c_str(), &mesh.obj) != C2B_OK) return mesh.fail_with(c2b_last_error());   // the message is per thread
        if (a.has("path")) {
            const std::string want = a.opt.at("path");
            std::string names;
            for (int64_t m = 0; m < c2b_obj_model_count(mesh.obj); ++m) {
                const std::string name = c2b_obj_model_name(mesh.obj, m);
                if (name == want && mesh.path_model < 0) mesh.path_model = m;
                names += (m ? ", " : "") + name;
            }
            if (mesh.path_model < 0) return mesh.fail_with("Could not find a path named " + want + ". Available model names are " + names);
        }
        if (a.has("move-to-origin") && c2b_obj_move_to_origin(mesh.obj, mesh.path_model) != C2B_OK) return mesh.fail_with(c2b_last_error());
        if (c2b_obj_triangles(mesh.obj, mesh.path_model, nullptr, &mesh.n_tri) != C2B_OK) return mesh.fail_with(c2b_last_error());
        mesh.tri.resize((size_t)mesh.n_tri * 9 + 1);
        if (c2b_obj_triangles(mesh.obj, mesh.path_model, mesh.tri.data(), &mesh.n_tri) != C2B_OK) return mesh.fail_with(c2b_last_error());
        mesh.want_bvh = mesh.n_tri >= 4096;                   // smaller meshes: the all-triangles kernel
        mesh.reach(1);
        if (mesh.want_bvh && mesh.path_model >= 0) build_bvh();
    });
    struct JoinWorker { std::thread &t; Mesh &m; ~JoinWorker() { if (t.joinable()) t.join(); if (m.bvh) c2b_bvh_free(m.bvh); } } join_worker{worker, mesh};
    c2b_problem *p = nullptr;
    const int create_rc = c2b_problem_create((int)a.i("device", 0), &p);
    const std::string create_err = create_rc != C2B_OK ? c2b_last_error() : "";
    mesh.wait_for(1);
    if (mesh.rc != C2B_OK) die(mesh.err);
    if (create_rc != C2B_OK) die(create_err);
    timer.mark("load .obj + triangles || HIP runtime start");
    c2b_obj *obj = mesh.obj;
    const int64_t path_model = mesh.path_model, n_tri = mesh.n_tri;
    const std::vector<float> &tri = mesh.tri;
    const bool own_bvh = mesh.want_bvh;

    int64_t n_cam = 0;
    std::vector<double> pos, dir;
    if (path_model >= 0) {
        n_cam = num_cameras;
        pos.resize((size_t)n_cam * 3 + 1); dir.resize((size_t)n_cam * 9 + 1);
        ck(c2b_generate_cameras_path(obj, path_model, num_cameras, step_size, seed, pos.data(), dir.data()));
    } else {
        // 2 * num_cameras disks at the densest packing bound the sample count (plus a rim for the open boundary)
        int64_t cap = 2 * num_cameras + 8 * (int64_t)std::sqrt((double)(2 * num_cameras)) + 64;
        pos.resize((size_t)cap * 3 + 1); dir.resize((size_t)cap * 9 + 1);
        // (the placement builds its own hierarchy for the downward rays while it throws its darts -- the longer of the
        // two; the one for the occlusion rays is started afterwards and hides behind the sampling and the sweep)
        ck(c2b_generate_cameras_poisson(tri.data(), n_tri, num_cameras, height, ground, seed, cap, pos.data(), dir.data(), &n_cam));
        if (n_cam > cap) {                                  // same seed => same cameras
            cap = n_cam;
            pos.resize((size_t)cap * 3 + 1); dir.resize((size_t)cap * 9 + 1);
            ck(c2b_generate_cameras_poisson(tri.data(), n_tri, num_cameras, height, ground, seed, cap, pos.data(), dir.data(), &n_cam));
        }
        if (own_bvh) {                                      // the worker has finished (stage 1 was its last): reuse the thread object
            worker.join();
            worker = std::thread(build_bvh);
        }
    }
    c2b_obj_free(obj);
    timer.mark("triangles + camera placement");
    std::printf("Generated %lld cameras\n", (long long)n_cam);

    HostProblem hp;
    hp.n_cam = n_cam;
    hp.cams15.resize((size_t)n_cam * 15 + 1);
    if (n_cam) ck(c2b_problem_from_position_direction(p, n_cam, pos.data(), dir.data(), hp.cams15.data()));
    ck(c2b_modify_intrinsics(hp.cams15.data(), n_cam, istart, iend, seed + 1));
    timer.mark("from_position_direction + intrinsics");
    std::printf("Modified intrinsics\n");

    std::vector<uint64_t> rows((size_t)n_cam + 1, 0);
    ck(c2b_problem_upload(p, n_cam, hp.cams15.data(), 0, nullptr, rows.data(), nullptr, nullptr));
    // generate_world_points_uniform on the resident cameras (r04: candidates evaluated on the device, the host sampler's
    // points bit for bit; C2B_HOST_SAMPLER=1 = the host sampler and a second upload)
    if (std::getenv("C2B_HOST_SAMPLER")) {
        std::vector<double> centers((size_t)n_cam * 3 + 1);
        if (n_cam) ck(c2b_problem_centers(p, centers.data()));
        hp.pts.resize((size_t)num_points * 3 + 1);
        ck(c2b_generate_world_points(tri.data(), n_tri, centers.data(), n_cam, num_points, max_dist, seed + 2, hp.pts.data(), &hp.n_pts));
        ck(c2b_problem_upload(p, n_cam, hp.cams15.data(), hp.n_pts, hp.pts.data(), rows.data(), nullptr, nullptr));
    } else {
        ck(c2b_problem_generate_world_points(p, tri.data(), n_tri, num_points, max_dist, seed + 2, &hp.n_pts));
    }
    timer.mark("world points");
    std::printf("Generated %lld world points\n", (long long)hp.n_pts);

    // visibility_graph, src/generate.rs:424-481: the points within max_dist of every camera that pass the predicate (the
    // cell list of the synthetic generators stands in for rstar here too since r04: the same lists as the brute-force
    // sweep of every camera against every point, 4x sooner at these sizes; C2B_DENSE_SWEEP=1 selects the sweep), then
    // the occlusion rays
    hp.row_ptr.assign((size_t)n_cam + 1, 0);
    if (std::getenv("C2B_DENSE_SWEEP")) ck(c2b_problem_visibility_dense(p, max_dist, hp.row_ptr.data()));
    else ck(c2b_problem_visibility_within_distance(p, max_dist, 0, 0.0, 0.0, hp.row_ptr.data()));
    timer.mark("candidates within max_dist + predicate");
    if (own_bvh) {
        mesh.wait_for(2);
        if (mesh.rc != C2B_OK) die(mesh.err);
        ck(c2b_problem_visibility_dense_occlude_bvh(p, mesh.bvh, hp.row_ptr.data()));
    } else {
        ck(c2b_problem_visibility_dense_occlude(p, tri.data(), n_tri, hp.row_ptr.data()));
    }
    timer.mark("occlusion rays + compaction (the hierarchy was built beside the phases above)");
    const size_t n_edges = (size_t)hp.row_ptr[(size_t)n_cam];
    std::printf("Computed visibility graph with %zu edges\n", n_edges);

    // from_visibility and cull stay on the device; one download at the end
    ck(c2b_problem_adopt_visibility(p));
    if (!a.has("no-lcc")) ck(c2b_problem_cull(p, a.has("exact-lcc") ? 0 : 1));
    timer.mark("from_visibility + cull (device)");
    int64_t nc = 0, np = 0, no = 0;
    ck(c2b_problem_sizes(p, &nc, &np, &no));
    if (nc == 0 || np == 0) die("EmptyProblem(\"No cameras remain\")");
    std::printf("Computed LCC with %lld cameras, %lld points, %lld edges\n", (long long)nc, (long long)np, (long long)no);

    double l1 = 0;
    ck(c2b_problem_total_reprojection_error(p, 1.0, &l1));
    std::printf("Total reprojection error: %s\n", display_f64(l1).c_str());
    timer.mark("error");
    // BAProblem::write of the resident problem: to_vec and a .bbal's file image on the device, nothing downloaded
    ck(c2b_problem_write(p, a.positional[1].c_str(), -1));
    timer.mark("write");
    c2b_problem_destroy(p);
    return 0;
}

// run_ply, src/bin/city2ba.rs:441-445
int run_ply(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    const HostBal h = read_bal(a.positional[0]);
    c2b_problem *p = nullptr;
    ck(create_problem((int)a.i("device", 0), &p));
    ck(upload_bal(p, h));
    std::vector<double> centers((size_t)h.n_cam * 3 + 1);
    ck(c2b_problem_centers(p, centers.data()));
    c2b_problem_destroy(p);
    ck(c2b_ply_write(a.positional[1].c_str(), h.n_cam, centers.data(), h.n_pts, h.pts.data(), h.row_ptr.data(), h.pt_idx.data()));
    return 0;
}

// The head `solve`, `triangulate` and `resect` share: read_problem, and the sizes printed (close_problem is their tail)
static c2b_problem *open_problem(PhaseTimer &timer, int device, const std::string &file, int64_t &nc, int64_t &np, int64_t &no) {
    c2b_problem *p = read_problem(timer, device, file);
    ck(c2b_problem_sizes(p, &nc, &np, &no));
    print_problem(nc, np, no);
    return p;
}

// `solve`: bundle adjustment of a .bal / .bbal by c2b_problem_levenberg_marquardt (an extension: the reference only makes
// problems).  The file is decoded into the resident problem, solved there and its image assembled there.  Every argument
// is parsed before the device is touched.  --filter-max-error X: --filter-rounds times (solve, then drop the observations
// whose residual exceeds X -- with --filter-in-front also those behind their camera), then one more solve with the loss
// cleared; cameras and points keep their numbers, nothing is culled.  --prior-from FILE: priors (c2b_problem_set_priors)
// whose targets are FILE's camera centres, intrinsics and points, weight 1 / sigma per component.

// sigmas of a --prior-*-sigma flag: `want` numbers (or also one, when `or_one`), each > 0; returned as weights 1 / sigma
static std::vector<double> prior_weights_of(const Args &a, const std::string &key, const char *shape, int want, bool or_one) {
    std::vector<double> w;
    const std::string bad = "Invalid value for '--" + key + " <" + shape + ">': expected " + shape + " with every sigma a number > 0";
    for (const std::string &part : split_commas(a.opt.at(key))) {
        char *end = nullptr;
        const double sigma = std::strtod(part.c_str(), &end);
        if (end == part.c_str() || *end || !(sigma > 0.0) || !std::isfinite(sigma)) die(bad);
        w.push_back(1.0 / sigma);
    }
    if (!((int)w.size() == want || (or_one && w.size() == 1))) die(bad);
    if ((int)w.size() < want) w.assign((size_t)want, w[0]);
    return w;
}

// n_cam and n_pts of a .bal / .bbal from its first line / header alone (no device, no parse of the body)
static void peek_counts(const std::string &path, int64_t &n_cam, int64_t &n_pts) {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) die("Could not open " + path);
    bool ok = false;
    if (path.size() >= 5 && path.compare(path.size() - 5, 5, ".bbal") == 0) {
        unsigned char b[16];
        ok = std::fread(b, 1, 16, f) == 16;
        uint64_t v[2] = {0, 0};
        for (int k = 0; k < 16; ++k) v[k / 8] = (v[k / 8] << 8) | b[k];
        n_cam = (int64_t)v[0]; n_pts = (int64_t)v[1];
    } else {
        long long c = 0, q = 0;
        ok = std::fscanf(f, "%lld %lld", &c, &q) == 2;
        n_cam = c; n_pts = q;
    }
    std::fclose(f);
    if (!ok) die("Could not read the camera and point counts of " + path);
}

// --loss, which `solve` and `refine` share: the kind (C2B loss kinds 0 .. 3)
static int loss_kind_of(const Args &a) {
    if (!a.has("loss")) return 0;
    const std::string &v = a.opt.at("loss");
    if (v == "squared") return 0;
    if (v == "huber") return 1;
    if (v == "cauchy") return 2;
    if (v == "soft-l1") return 3;
    die("Invalid value for '--loss <loss>': expected squared, huber, cauchy or soft-l1");
}

int run_solve(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"fix-intrinsics", "fix-first-camera", "filter-in-front", "no-halo"},
                         {"iterations", "lambda", "pcg-iterations", "pcg-tol", "function-tol", "gradient-tol", "parameter-tol", "loss",
                          "loss-scale", "preconditioner", "schur", "linear-solver", "inner-iterations", "device", "filter-max-error", "filter-rounds", "prior-from",
                          "prior-center-sigma", "prior-intrinsics-sigma", "prior-point-sigma", "prior-point-every", "window", "window-around", "hops",
                          "min-shared", "max-cameras"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    c2b_lm_options opt;
    opt.max_iterations = (int32_t)std::min<int64_t>(a.i("iterations", 10), 1 << 20);
    opt.pcg_max_iters = (int32_t)std::min<int64_t>(a.i("pcg-iterations", 100), 1 << 20);
    opt.lambda0 = a.f("lambda", 1e-4);
    opt.pcg_rel_tol = a.f("pcg-tol", 1e-6);
    opt.function_tol = a.f("function-tol", 0.0);
    opt.gradient_tol = a.f("gradient-tol", 0.0);
    opt.parameter_tol = a.f("parameter-tol", 0.0);
    const double loss_scale = a.f("loss-scale", 1.0);
    const int device = (int)a.i("device", 0);
    const bool filter = a.has("filter-max-error");
    const double filter_max_error = a.f("filter-max-error", 0.0);
    const int64_t filter_rounds = a.i("filter-rounds", 1);
    const int filter_flags = a.has("filter-in-front") ? C2B_FILTER_IN_FRONT : 0;
    if (filter && !(filter_max_error >= 0.0)) die("Invalid value for '--filter-max-error <X>': expected a number >= 0");
    if (filter_rounds > 1000) die("Invalid value for '--filter-rounds <N>': expected 0 ... 1000");
    if (!filter && (a.has("filter-rounds") || a.has("filter-in-front"))) die("--filter-rounds and --filter-in-front need --filter-max-error <X>");
    const int loss = loss_kind_of(a);
    int precond = C2B_PRECOND_BLOCK_JACOBI;
    if (a.has("preconditioner")) {
        const std::string &v = a.opt.at("preconditioner");
        if (v == "block-jacobi") precond = C2B_PRECOND_BLOCK_JACOBI;
        else if (v == "schur-jacobi") precond = C2B_PRECOND_SCHUR_JACOBI;
        else die("Invalid value for '--preconditioner <preconditioner>': expected block-jacobi or schur-jacobi");
    }
    int schur = C2B_SCHUR_IMPLICIT;
    if (a.has("schur")) {
        const std::string &v = a.opt.at("schur");
        if (v == "implicit") schur = C2B_SCHUR_IMPLICIT;
        else if (v == "explicit") schur = C2B_SCHUR_EXPLICIT;
        else die("Invalid value for '--schur <implicit|explicit>': expected implicit or explicit");
    }
    int linear = C2B_LINEAR_PCG;
    if (a.has("linear-solver")) {
        const std::string &v = a.opt.at("linear-solver");
        if (v == "pcg") linear = C2B_LINEAR_PCG;
        else if (v == "cholesky") linear = C2B_LINEAR_CHOLESKY;
        else die("Invalid value for '--linear-solver <pcg|cholesky>': expected pcg or cholesky");
    }
    const int64_t inner_iterations = a.i("inner-iterations", 0);
    if (inner_iterations > 1000) die("Invalid value for '--inner-iterations <N>': expected an integer in 0 ... 1000");
    // --window LO:HI: cameras LO .. HI - 1 are solved with their rim held constant; the range is checked against the file's
    // camera count here, before a device exists
    const bool window = a.has("window");
    int64_t win_lo = 0, win_hi = 0;
    // --window-around C[,C...]: the cameras within --hops edges of the covisibility graph at --min-shared, at most --max-cameras
    const bool around = a.has("window-around");
    if (window && around) die("--window <LO:HI> and --window-around <C[,C...]> cannot be used together");
    if (a.has("no-halo") && !window && !around) die("--no-halo needs --window <LO:HI> or --window-around <C[,C...]>");
    for (const char *k : {"hops", "min-shared", "max-cameras"})
        if (a.has(k) && !around) die(std::string("--") + k + " needs --window-around <C[,C...]>");
    std::vector<int64_t> around_cams;
    const int64_t hops = a.i("hops", 1), min_shared = a.i("min-shared", 1), max_cameras = a.i("max-cameras", 0);
    if (around) {
        const std::string &v = a.opt.at("window-around");
        const std::string bad = "Invalid value for '--window-around <C[,C...]>': expected camera indices separated by commas";
        size_t at = 0;
        while (at <= v.size()) {
            const size_t comma = std::min(v.find(',', at), v.size());
            if (comma == at || comma - at > 18) die(bad);
            for (size_t k = at; k < comma; ++k)
                if (v[k] < '0' || v[k] > '9') die(bad);
            around_cams.push_back(std::stoll(v.substr(at, comma - at)));
            at = comma + 1;
        }
        if (hops < 0 || hops > 2147483647) die("Invalid value for '--hops <N>': expected an integer >= 0");
        if (min_shared < 1 || min_shared > 2147483647) die("Invalid value for '--min-shared <K>': expected an integer >= 1");
        if (a.has("max-cameras") && max_cameras < (int64_t)around_cams.size())
            die("Invalid value for '--max-cameras <M>': expected at least the number of cameras given to --window-around");
        int64_t in_cam = 0, in_pts = 0;
        peek_counts(a.positional[0], in_cam, in_pts);
        for (const int64_t c : around_cams)
            if (c >= in_cam)
                die("--window-around: " + a.positional[0] + " has " + std::to_string(in_cam) + " cameras, camera " + std::to_string(c) + " was given");
    }
    if (window) {
        const std::string &v = a.opt.at("window");
        const std::string bad = "Invalid value for '--window <LO:HI>': expected two integers LO:HI with 0 <= LO < HI <= the number of cameras";
        const size_t colon = v.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 == v.size()) die(bad);
        for (size_t k = 0; k < v.size(); ++k)
            if (k != colon && (v[k] < '0' || v[k] > '9')) die(bad);
        if (colon > 18 || v.size() - colon - 1 > 18) die(bad);
        win_lo = std::stoll(v.substr(0, colon));
        win_hi = std::stoll(v.substr(colon + 1));
        if (win_lo >= win_hi) die(bad);
        int64_t in_cam = 0, in_pts = 0;
        peek_counts(a.positional[0], in_cam, in_pts);
        if (win_hi > in_cam)
            die("--window: " + a.positional[0] + " has " + std::to_string(in_cam) + " cameras, the window ends at " + std::to_string(win_hi));
    }
    // priors: every flag and both files' counts are checked here, before a device exists
    const bool prior = a.has("prior-from");
    std::vector<double> w_center, w_intr, w_point;
    int64_t point_every = 1;
    for (const char *k : {"prior-center-sigma", "prior-intrinsics-sigma", "prior-point-sigma", "prior-point-every"})
        if (a.has(k) && !prior) die(std::string("--") + k + " needs --prior-from <FILE>");
    if (prior) {
        if (a.has("prior-center-sigma")) w_center = prior_weights_of(a, "prior-center-sigma", "S|SX,SY,SZ", 3, true);
        if (a.has("prior-intrinsics-sigma")) w_intr = prior_weights_of(a, "prior-intrinsics-sigma", "SF,SK1,SK2", 3, false);
        if (a.has("prior-point-sigma")) w_point = prior_weights_of(a, "prior-point-sigma", "S", 3, true);
        if (w_point.size() == 3 && a.opt.at("prior-point-sigma").find(',') != std::string::npos)
            die("Invalid value for '--prior-point-sigma <S>': expected S with every sigma a number > 0");
        if (w_center.empty() && w_intr.empty() && w_point.empty())
            die("--prior-from <FILE> needs at least one of --prior-center-sigma, --prior-intrinsics-sigma, --prior-point-sigma");
        if (a.has("prior-point-every")) {
            if (w_point.empty()) die("--prior-point-every needs --prior-point-sigma <S>");
            point_every = a.i("prior-point-every", 1);
            if (point_every < 1) die("Invalid value for '--prior-point-every <N>': expected N >= 1");
        }
        int64_t in_cam = 0, in_pts = 0, from_cam = 0, from_pts = 0;
        peek_counts(a.positional[0], in_cam, in_pts);
        peek_counts(a.opt.at("prior-from"), from_cam, from_pts);
        if (from_cam != in_cam)
            die("--prior-from: " + a.opt.at("prior-from") + " has " + std::to_string(from_cam) + " cameras, " + a.positional[0] + " has " +
                std::to_string(in_cam));
        if (!w_point.empty() && from_pts != in_pts)
            die("--prior-from: " + a.opt.at("prior-from") + " has " + std::to_string(from_pts) + " points, " + a.positional[0] + " has " +
                std::to_string(in_pts) + " (a point prior needs the same points)");
    }
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    ck(c2b_problem_set_loss(p, loss, loss_scale));
    ck(c2b_problem_set_preconditioner(p, precond));
    ck(c2b_problem_set_schur(p, schur));
    ck(c2b_problem_set_linear_solver(p, linear));
    ck(c2b_problem_set_inner_iterations(p, (int)inner_iterations));
    if (prior) {                                             // the targets: FILE's centres, intrinsics and points, as a problem holds them
        c2b_problem *q = nullptr;
        int64_t qc = 0, qp = 0, qo = 0;
        ck(create_problem(device, &q));
        ck(c2b_problem_read(q, a.opt.at("prior-from").c_str(), -1));
        ck(c2b_problem_sizes(q, &qc, &qp, &qo));
        if (qc != nc || (!w_point.empty() && qp != np)) die("--prior-from: the counts of " + a.opt.at("prior-from") + " are not those of " + a.positional[0]);
        std::vector<double> c0((size_t)nc * 3 + 1), b9((size_t)nc * 9 + 1), x0((size_t)qp * 3 + 1), cams15((size_t)nc * 15 + 1);
        ck(c2b_problem_centers(q, c0.data()));
        ck(c2b_problem_download_bal(q, b9.data()));
        ck(c2b_problem_download(q, cams15.data(), x0.data(), nullptr));
        c2b_problem_destroy(q);
        std::vector<double> i0((size_t)nc * 3 + 1), cw, iw, xw;
        for (int64_t c = 0; c < nc; ++c)
            for (int k = 0; k < 3; ++k) i0[(size_t)(3 * c + k)] = b9[(size_t)(9 * c + 6 + k)];
        auto spread = [](const std::vector<double> &w3, int64_t n, int64_t every) {
            std::vector<double> w((size_t)n * 3 + 1, 0.0);
            for (int64_t i = 0; i < n; i += every)
                for (int k = 0; k < 3; ++k) w[(size_t)(3 * i + k)] = w3[(size_t)k];
            return w;
        };
        if (!w_center.empty()) cw = spread(w_center, nc, 1);
        if (!w_intr.empty()) iw = spread(w_intr, nc, 1);
        if (!w_point.empty()) xw = spread(w_point, np, point_every);
        ck(c2b_problem_set_priors(p, cw.empty() ? nullptr : c0.data(), cw.empty() ? nullptr : cw.data(), iw.empty() ? nullptr : i0.data(),
                                  iw.empty() ? nullptr : iw.data(), xw.empty() ? nullptr : x0.data(), xw.empty() ? nullptr : xw.data()));
        timer.mark("priors (targets read on the device, c2b_problem_set_priors)");
    }
    if (a.has("fix-intrinsics") || a.has("fix-first-camera")) {
        std::vector<c2b_camera_mask> cm((size_t)nc + 1, (c2b_camera_mask)(a.has("fix-intrinsics") ? C2B_CONST_INTRINSICS : 0));
        if (a.has("fix-first-camera") && nc) cm[0] |= C2B_CONST_POSE;
        ck(c2b_problem_set_constant(p, cm.data(), nullptr));
    }
    // the window: a child of the problem that carries everything set above (the rim's masks on top); it is what is solved
    c2b_problem *whole = p;
    if (window || around) {
        std::vector<uint8_t> seed((size_t)nc + 1, 0);
        for (int64_t c = win_lo; c < win_hi && c < nc; ++c) seed[(size_t)c] = 1;
        if (around) {
            std::vector<uint8_t> from((size_t)nc + 1, 0);
            for (const int64_t c : around_cams)
                if (c < nc) from[(size_t)c] = 1;
            int64_t members = 0;
            ck(c2b_problem_neighbourhood(whole, from.data(), (int)hops, (int)min_shared, max_cameras, nullptr, seed.data(), nullptr, &members));
            timer.mark("neighbourhood (device)");
            std::printf("neighbourhood of %lld cameras: %lld hops at %lld shared points: %lld cameras\n", (long long)around_cams.size(), (long long)hops,
                        (long long)min_shared, (long long)members);
        }
        c2b_problem *child = nullptr;
        ck(create_problem(device, &child));
        ck(c2b_problem_window(whole, seed.data(), a.has("no-halo") ? 0 : C2B_WINDOW_HALO, child));
        p = child;
        ck(c2b_problem_sizes(p, &nc, &np, &no));
        timer.mark("window (device)");
        if (window)
            std::printf("window %lld:%lld: %lld cameras, %lld points, %lld observations\n", (long long)win_lo, (long long)win_hi, (long long)nc,
                        (long long)np, (long long)no);
        else
            std::printf("window: %lld cameras, %lld points, %lld observations\n", (long long)nc, (long long)np, (long long)no);
    }
    std::vector<c2b_lm_iteration> hist((size_t)opt.max_iterations + 1);
    static const char *const why[] = {"iteration limit reached", "function tolerance reached", "gradient tolerance reached",
                                      "parameter tolerance reached", "cost or gradient not finite"};
    auto solve_once = [&]() {
        c2b_lm_summary sum;
        ck(c2b_problem_levenberg_marquardt(p, &opt, hist.data(), (int)hist.size(), &sum));
        timer.mark("levenberg_marquardt (device)");
        for (int k = 0; k < sum.iterations; ++k) {
            const c2b_lm_iteration &it = hist[(size_t)k];
            std::printf("iteration %d: cost %.17g lambda %.6e %s pcg %d\n", k, it.cost, it.lambda, it.accepted ? "accepted" : "rejected", it.pcg_iterations);
        }
        std::printf("Termination: %s after %d iterations; cost %.17g -> %.17g\n", why[sum.termination], sum.iterations, sum.initial_cost, sum.final_cost);
    };
    if (filter) {
        for (int64_t round = 0; round < filter_rounds; ++round) {
            solve_once();
            int64_t removed = 0;
            ck(c2b_problem_filter_observations(p, filter_max_error, filter_flags, &removed));
            ck(c2b_problem_sizes(p, &nc, &np, &no));
            timer.mark("filter_observations (device)");
            std::printf("filter round %lld: removed %lld observations, %lld left\n", (long long)round, (long long)removed, (long long)no);
        }
        ck(c2b_problem_set_loss(p, 0, 1.0));
    }
    solve_once();
    if (window || around) {                                  // the child's free cameras and points back into the whole problem
        int64_t wc = 0, wp = 0;
        ck(c2b_problem_write_back(p, whole, &wc, &wp));
        c2b_problem_destroy(p);
        p = whole;
        timer.mark("write_back (device)");
        std::printf("written back: %lld cameras, %lld points\n", (long long)wc, (long long)wp);
    }
    close_problem(timer, p, a.positional[1]);
    return 0;
}

// `covisibility IN [--min-shared K]`: the camera covisibility graph's figures, one line
int run_covisibility(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"min-shared", "device"});
    if (a.positional.size() != 1) die("The following required arguments were not provided:\n    <FILE>");
    const int64_t min_shared = a.i("min-shared", 1);
    if (min_shared < 1 || min_shared > 2147483647) die("Invalid value for '--min-shared <K>': expected an integer >= 1");
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0, edges = 0;
    c2b_problem *p = open_problem(timer, (int)a.i("device", 0), a.positional[0], nc, np, no);
    ck(c2b_problem_covisibility(p, (int)min_shared, &edges));
    std::vector<uint64_t> ptr((size_t)nc + 1, 0);
    ck(c2b_problem_get_covisibility(p, ptr.data(), nullptr, nullptr, nullptr, nullptr));
    timer.mark("covisibility (device)");
    uint64_t max_degree = 0;
    int64_t isolated = 0;
    for (int64_t c = 0; c < nc; ++c) {
        const uint64_t d = ptr[(size_t)c + 1] - ptr[(size_t)c];
        max_degree = std::max(max_degree, d);
        isolated += d == 0;
    }
    std::printf("covisibility at %lld shared points: %lld cameras, %lld edges, maximum degree %llu, %lld isolated cameras\n", (long long)min_shared,
                (long long)nc, (long long)(edges / 2), (unsigned long long)max_degree, (long long)isolated);
    c2b_problem_destroy(p);
    return 0;
}

// `compare EST REF`: how close EST came to REF -- the same cameras and points under the same indices -- after the best similarity
// between their frames (c2b_problem_align): ONE JSON line with the transform, the status and the two summaries.
// --apply OUT writes EST moved into REF's frame.  Every argument is parsed before the device is touched.  (Priors are a handle's
// state and no file carries them, so there is none here for the transform to leave behind.)
int run_compare(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"no-scale"}, {"on", "max-dist", "rounds", "apply", "device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <EST> <REF>");
    const std::string on = a.has("on") ? a.opt.at("on") : "cameras";
    if (on != "cameras" && on != "points" && on != "both") die("Invalid value for '--on <KIND>': expected cameras, points or both");
    const double max_dist = a.f("max-dist", 0.0);
    if (a.has("max-dist") && !(max_dist > 0.0 && std::isfinite(max_dist))) die("Invalid value for '--max-dist <D>': expected a finite number > 0");
    const int64_t rounds = a.i("rounds", 5);
    if (rounds < 1 || rounds > 2147483647) die("Invalid value for '--rounds <N>': expected an integer >= 1");
    if (a.has("rounds") && !a.has("max-dist")) die("--rounds needs --max-dist <D>");
    PhaseTimer timer;
    const int device = (int)a.i("device", 0);
    c2b_problem *est = read_problem(timer, device, a.positional[0]), *ref = read_problem(timer, device, a.positional[1]);
    c2b_align_options o;
    c2b_align_options_init(&o);
    o.on = on == "cameras" ? C2B_ALIGN_CAMERAS : (on == "points" ? C2B_ALIGN_POINTS : C2B_ALIGN_BOTH);
    o.scale = a.has("no-scale") ? 0 : 1;
    o.max_dist = max_dist;
    o.rounds = a.has("max-dist") ? (int)rounds : 0;
    c2b_similarity T;
    c2b_align_summary S;
    ck(c2b_problem_align(est, ref, &o, &T, &S, nullptr, nullptr, nullptr, nullptr, nullptr));
    timer.mark("align (device)");
    static const char *const status[] = {"ok", "too_few", "degenerate"};
    auto stat = [](const c2b_align_stat &s, double unit) {
        char buf[256];
        const double n = (double)s.n;
        std::snprintf(buf, sizeof buf, "{\"n\": %lld, \"rmse\": %.17g, \"mean\": %.17g, \"max\": %.17g, \"argmax\": %lld}", (long long)s.n,
                      s.n ? unit * std::sqrt(s.sum_sq / n) : 0.0, s.n ? unit * s.sum / n : 0.0, s.n ? unit * s.max : 0.0, (long long)s.argmax);
        return std::string(buf);
    };
    std::printf("{\"status\": \"%s\", \"rounds\": %d, \"scale\": %.17g, \"rotation\": [[%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g], [%.17g, %.17g, %.17g]], "
                "\"translation\": [%.17g, %.17g, %.17g], \"cameras\": %s, \"camera_rotations_deg\": %s, \"points\": %s}\n",
                status[S.status], S.rounds, T.scale, T.rotation[0], T.rotation[1], T.rotation[2], T.rotation[3], T.rotation[4], T.rotation[5], T.rotation[6],
                T.rotation[7], T.rotation[8], T.translation[0], T.translation[1], T.translation[2], stat(S.cameras, 1.0).c_str(),
                stat(S.camera_rotations, 180.0 / 3.14159265358979323846).c_str(), stat(S.points, 1.0).c_str());
    c2b_problem_destroy(ref);
    if (a.has("apply")) {
        ck(c2b_problem_transform(est, &T));
        timer.mark("transform (device)");
        close_problem(timer, est, a.opt.at("apply"));
    } else {
        c2b_problem_destroy(est);
    }
    return 0;
}

// The consensus flags `triangulate` and `resect` share, parsed and cross-checked: --min-inliers is at least `least`, `dflt`
// when absent.
struct Consensus { bool on, drop_outliers; double max_error; int min_inliers, max_hypotheses; };

static Consensus consensus_of(const Args &a, int64_t least, int64_t dflt) {
    Consensus c = {a.has("max-error"), a.has("drop-outliers"), a.f("max-error", 0.0), 0, 0};
    const int64_t min_inliers = a.i("min-inliers", dflt), max_hypotheses = a.i("max-hypotheses", 64);
    if (c.on && !(c.max_error >= 0.0 && std::isfinite(c.max_error))) die("Invalid value for '--max-error <X>': expected a finite number >= 0");
    if (min_inliers < least || min_inliers > 2147483647) die("Invalid value for '--min-inliers <N>': expected an integer of at least " + std::to_string(least));
    if (max_hypotheses < 1 || max_hypotheses > 64) die("Invalid value for '--max-hypotheses <H>': expected an integer in 1 ... 64");
    if (!c.on && (a.has("min-inliers") || a.has("max-hypotheses") || c.drop_outliers))
        die("--min-inliers, --max-hypotheses and --drop-outliers need --max-error <X>");
    c.min_inliers = (int)min_inliers; c.max_hypotheses = (int)max_hypotheses;
    return c;
}

// What a start-up pass did, from its counts: "<did> N <what>; kept: ..." -- with `inlier` (consensus) also the count
// without consensus and a second line.  C2B_TRI_* and C2B_RES_* number the outcomes alike.
static_assert(C2B_TRI_OK == C2B_RES_OK && C2B_TRI_TOO_FEW == C2B_RES_TOO_FEW && C2B_TRI_DEGENERATE == C2B_RES_DEGENERATE &&
              C2B_TRI_BEHIND == C2B_RES_BEHIND && C2B_TRI_CONSTANT == C2B_RES_CONSTANT && C2B_TRI_NO_CONSENSUS == C2B_RES_NO_CONSENSUS, "");
static void print_summary(const char *did, const char *what, const char *behind, const int64_t counts[6], const std::vector<uint8_t> *inlier,
                          int64_t removed) {
    std::printf("%s %lld %s; kept: %lld too few observations, %lld degenerate, %lld behind a %s, %lld constant", did, (long long)counts[C2B_TRI_OK],
                what, (long long)counts[C2B_TRI_TOO_FEW], (long long)counts[C2B_TRI_DEGENERATE], (long long)counts[C2B_TRI_BEHIND], behind,
                (long long)counts[C2B_TRI_CONSTANT]);
    if (inlier)
        std::printf(", %lld without consensus\n%lld outlier observations, %lld removed", (long long)counts[C2B_TRI_NO_CONSENSUS],
                    (long long)std::count(inlier->begin(), inlier->end(), (uint8_t)0), (long long)removed);
    std::printf("\n");
}

// `triangulate`: every point of a .bal / .bbal from its cameras and observations by c2b_problem_triangulate_points (an
// extension: linear midpoint triangulation on the device; cameras and observations are written as they were read).  Every
// argument is parsed before the device is touched.  --max-error X selects consensus triangulation
// (c2b_problem_triangulate_consensus): candidates from pairs of rays, the one most observations reproject within X of, a
// refit on those; --drop-outliers then removes the other observations of the triangulated points from the list.
int run_triangulate(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"drop-outliers"}, {"min-angle", "device", "max-error", "min-inliers", "max-hypotheses"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    const double min_angle_deg = a.f("min-angle", 1.0);
    const int device = (int)a.i("device", 0);
    if (!(min_angle_deg >= 0.0 && min_angle_deg <= 90.0)) die("Invalid value for '--min-angle <DEG>': expected a number in 0 ... 90");
    const double min_angle = min_angle_deg * (3.14159265358979323846 / 180.0);
    const Consensus c = consensus_of(a, 2, 3);
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}, removed = 0;
    std::vector<uint8_t> inlier((size_t)(c.on ? no : 0));
    ck(c.on ? c2b_problem_triangulate_consensus(p, min_angle, c.max_error, c.min_inliers, c.max_hypotheses, c.drop_outliers ? C2B_TRI_DROP_OUTLIERS : 0,
                                                nullptr, nullptr, inlier.data(), counts, &removed)
            : c2b_problem_triangulate_points(p, min_angle, nullptr, counts));
    timer.mark(c.on ? "triangulate_consensus (device)" : "triangulate_points (device)");
    print_summary("triangulated", "points", "camera", counts, c.on ? &inlier : nullptr, removed);
    close_problem(timer, p, a.positional[1]);
    return 0;
}

// `resect`: every camera pose of a .bal / .bbal from its points and observations by c2b_problem_resect_cameras (an
// extension: the minimiser of the object-space error on the device; points, intrinsics and observations are written as they
// were read).  Every argument is parsed before the device is touched.  --max-error X selects consensus resection
// (c2b_problem_resect_consensus): candidate poses from triples of observations, the one most observations reproject within
// X of, the same fit on those; --drop-outliers then removes the other observations of the resected cameras from the list.
int run_resect(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"drop-outliers"}, {"min-points", "min-gap", "device", "max-error", "min-inliers", "max-hypotheses"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    const int64_t min_points = a.i("min-points", 6);
    const double min_gap = a.f("min-gap", 1e-4);
    const int device = (int)a.i("device", 0);
    if (min_points < 6 || min_points > 2147483647) die("Invalid value for '--min-points <N>': expected an integer of at least 6");
    if (!(min_gap >= 0.0 && min_gap < 1.0)) die("Invalid value for '--min-gap <G>': expected a number in 0 ... 1 (1 excluded)");
    const Consensus c = consensus_of(a, 6, 6);
    if (c.on && a.has("min-points")) die("--min-points does not go with --max-error <X>: --min-inliers <N> takes its place");
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}, removed = 0;
    std::vector<uint8_t> inlier((size_t)(c.on ? no : 0));
    ck(c.on ? c2b_problem_resect_consensus(p, c.max_error, c.min_inliers, min_gap, c.max_hypotheses, c.drop_outliers ? C2B_RES_DROP_OUTLIERS : 0,
                                           nullptr, nullptr, nullptr, inlier.data(), counts, &removed)
            : c2b_problem_resect_cameras(p, (int)min_points, min_gap, nullptr, counts));
    timer.mark(c.on ? "resect_consensus (device)" : "resect_cameras (device)");
    print_summary("resected", "cameras", "point", counts, c.on ? &inlier : nullptr, removed);
    close_problem(timer, p, a.positional[1]);
    return 0;
}

// `merge`: duplicate landmarks of a .bal / .bbal merged by c2b_problem_merge_points (an extension: the repair of
// `noise --split-landmarks` and of broken tracks; cameras and observed pixels are written as they were read).  Every argument
// is parsed before the device is touched.  The absorbed points stay in the file as unobserved points: nothing is culled.
int run_merge(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"radius", "max-error", "rounds", "device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    if (!a.has("radius") || !a.has("max-error")) die("The following required arguments were not provided:\n    --radius <R> --max-error <X>");
    const double radius = a.f("radius", 0.0), max_error = a.f("max-error", 0.0);
    const int64_t rounds = a.i("rounds", 1);
    const int device = (int)a.i("device", 0);
    if (!(radius >= 0.0 && std::isfinite(radius))) die("Invalid value for '--radius <R>': expected a finite number >= 0");
    if (!(max_error >= 0.0 && std::isfinite(max_error))) die("Invalid value for '--max-error <X>': expected a finite number >= 0");
    if (rounds < 1 || rounds > 1000) die("Invalid value for '--rounds <N>': expected an integer in 1 ... 1000");
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0, merged = 0;
    int run = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    ck(c2b_problem_merge_points(p, radius, max_error, (int)rounds, nullptr, &merged, &run));
    timer.mark("merge_points (device)");
    std::printf("merged %lld points in %d rounds; they stay in the file as unobserved points\n", (long long)merged, run);
    close_problem(timer, p, a.positional[1]);
    return 0;
}

// `rematch`: the wrong point indices of a .bal / .bbal put right by c2b_problem_rematch_observations (an extension: the repair
// of `noise --mismatch-chance` and `--join-landmarks` that keeps the measurement; cameras, points and the surviving pixels are
// written as they were read).  Every argument is parsed before the device is touched.  Nothing is culled.
int run_rematch(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {}, {"radius", "max-error", "min-fits", "device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    if (!a.has("radius") || !a.has("max-error")) die("The following required arguments were not provided:\n    --radius <R> --max-error <X>");
    const double radius = a.f("radius", 0.0), max_error = a.f("max-error", 0.0);
    const int64_t min_fits = a.i("min-fits", 2);
    const int device = (int)a.i("device", 0);
    if (!(radius >= 0.0 && std::isfinite(radius))) die("Invalid value for '--radius <R>': expected a finite number >= 0");
    if (!(max_error >= 0.0 && std::isfinite(max_error))) die("Invalid value for '--max-error <X>': expected a finite number >= 0");
    if (min_fits > 1000000) die("Invalid value for '--min-fits <N>': expected an integer in 0 ... 1000000");      // (the parser refuses a negative one)
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0, reassigned = 0, removed = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    ck(c2b_problem_rematch_observations(p, radius, max_error, (int)min_fits, nullptr, &reassigned, &removed));
    timer.mark("rematch_observations (device)");
    std::printf("reassigned %lld observations and removed %lld of %lld; nothing is culled\n", (long long)reassigned, (long long)removed, (long long)no);
    close_problem(timer, p, a.positional[1]);
    return 0;
}

// `refine`: every point of a .bal / .bbal re-minimised by itself against the cameras as they are, by
// c2b_problem_refine_points (an extension: per-point Levenberg-Marquardt on the device; cameras and observations are written as
// they were read); with --cameras every camera against the points as they are, by c2b_problem_refine_cameras (the points are
// written as they were read); with --alternate N, N sweeps of both, cameras first.  Every argument is parsed before the device
// is touched.
void print_refined(const char *what, const int64_t counts[6]) {
    std::printf("refined %lld %s: %lld converged, %lld at the round limit; kept: %lld unobserved, %lld with a cost that is not finite, %lld constant\n",
                (long long)counts[5], what, (long long)counts[C2B_REFINE_CONVERGED], (long long)counts[C2B_REFINE_MAX_ROUNDS],
                (long long)counts[C2B_REFINE_UNOBSERVED], (long long)counts[C2B_REFINE_FAILED], (long long)counts[C2B_REFINE_CONSTANT]);
}

int run_refine(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {"cameras"},
                         {"rounds", "lambda", "loss", "loss-scale", "function-tol", "gradient-tol", "parameter-tol", "alternate", "device"});
    if (a.positional.size() != 2) die("The following required arguments were not provided:\n    <FILE> <OUT>");
    if (a.has("cameras") && a.has("alternate")) die("The argument '--cameras' cannot be used with '--alternate <N>'");
    const int64_t sweeps = a.i("alternate", 0);
    if (sweeps > 1000000) die("Invalid value for '--alternate <N>': expected an integer in 0 ... 1000000");
    const int64_t rounds = a.i("rounds", 10);
    if (rounds > 1000000) die("Invalid value for '--rounds <N>': expected an integer in 0 ... 1000000");
    c2b_refine_options opt = {(int32_t)rounds, 0, a.f("lambda", 1e-4), a.f("function-tol", 0.0), a.f("gradient-tol", 0.0), a.f("parameter-tol", 0.0)};
    if (!(opt.lambda0 >= C2B_STEP_LAMBDA_MIN && opt.lambda0 <= C2B_STEP_LAMBDA_MAX)) die("Invalid value for '--lambda <L>': expected a number in 1e-20 ... 1e32");
    const std::pair<const char *, double> tols[] = {{"function-tol", opt.function_tol}, {"gradient-tol", opt.gradient_tol}, {"parameter-tol", opt.parameter_tol}};
    for (const auto &t : tols)
        if (!(t.second >= 0.0 && std::isfinite(t.second))) die(std::string("Invalid value for '--") + t.first + " <T>': expected a finite number >= 0");
    const int loss = loss_kind_of(a);
    const double loss_scale = a.f("loss-scale", 1.0);
    if (!(loss_scale > 0.0 && std::isfinite(loss_scale))) die("Invalid value for '--loss-scale <A>': expected a finite number > 0");
    const int device = (int)a.i("device", 0);
    PhaseTimer timer;
    int64_t nc = 0, np = 0, no = 0;
    c2b_problem *p = open_problem(timer, device, a.positional[0], nc, np, no);
    ck(c2b_problem_set_loss(p, loss, loss_scale));
    int64_t counts[6] = {0, 0, 0, 0, 0, 0};
    if (a.has("alternate")) {                                // the last sweep's counts are the ones reported
        int64_t cam_counts[6] = {0, 0, 0, 0, 0, 0};
        for (int64_t s = 0; s < sweeps; ++s) {
            ck(c2b_problem_refine_cameras(p, &opt, nullptr, cam_counts));
            ck(c2b_problem_refine_points(p, &opt, nullptr, counts));
        }
        timer.mark("refine_cameras / refine_points (device)");
        std::printf("%lld sweeps; the last one:\n", (long long)sweeps);
        print_refined("cameras", cam_counts);
        print_refined("points", counts);
    } else if (a.has("cameras")) {
        ck(c2b_problem_refine_cameras(p, &opt, nullptr, counts));
        timer.mark("refine_cameras (device)");
        print_refined("cameras", counts);
    } else {
        ck(c2b_problem_refine_points(p, &opt, nullptr, counts));
        timer.mark("refine_points (device)");
        print_refined("points", counts);
    }
    close_problem(timer, p, a.positional[1]);
    return 0;
}

void usage() {
    std::printf("city2ba (MI355X build, %s)\nTools for generating synthetic bundle adjustment problems.\n\n"
                "USAGE:\n    city2ba <SUBCOMMAND>\n\nSUBCOMMANDS:\n"
                "    synthetic         Generate a synthetic bundle adjustment problem from an grid of city blocks.\n"
                "    synthetic-line    Generate a synthetic bundle adjustment problem on a line.\n"
                "    noise             Add noise to a bundle adjustment problem.\n"
                "    generate          Generate a synthetic bundle adjustment problem from a 3D model.\n"
                "    ply               Convert a .bal or .bbal to a .ply for visualization.\n"
                "    solve             Bundle-adjust a .bal or .bbal by Levenberg-Marquardt on the device.\n"
                "    covisibility      Print the figures of the camera covisibility graph of a .bal or .bbal.\n"
                "    compare           Align a .bal or .bbal to its ground truth by a similarity and print the errors that remain.\n"
                "    triangulate       Set the points of a .bal or .bbal from its cameras and observations.\n"
                "    resect            Set the camera poses of a .bal or .bbal from its points and observations.\n"
                "    merge             Merge the duplicate landmarks of a .bal or .bbal (the repair of noise --split-landmarks).\n"
                "    rematch           Put the wrong point indices of a .bal or .bbal right (the repair of noise --mismatch-chance).\n"
                "    refine            Refine every point (or, --cameras, every camera) of a .bal or .bbal by itself, the rest held.\n",
                c2b_version());
}

// flags of each subcommand with the reference's defaults (src/bin/city2ba.rs:33-260)
const char *subcommand_help(const std::string &sub) {
    if (sub == "synthetic")
        return "city2ba synthetic <OUTPUT>\n"
               "    --blocks <N>              city blocks per side [5]\n"
               "    --cameras-per-block <N>   [10]        --points-per-block <N>   [10]\n"
               "    --block-length <X>        [20]        --block-inset <X>        [1]\n"
               "    --camera-height <X>       [1]         --point-height <X>       [1]\n"
               "    --max-dist <X>            maximum camera-point distance [10]\n";
    if (sub == "synthetic-line")
        return "city2ba synthetic-line <OUTPUT>\n"
               "    --cameras <N> [10]   --points <N> [10]   --length <X> [20]   --point-offset <X> [1]\n"
               "    --camera-height <X> [1]   --point-height <X> [1]   --max-dist <X> [10]\n";
    if (sub == "noise")
        return "city2ba noise <FILE> <OUT>\n"
               "    --rotation-std <X> --translation-std <X> --point-std <X> --observation-std <X>   Gaussian noise [0]\n"
               "    --drift-strength <X> --drift-angle <X> --drift-std <X> [--fixed-drift]            drift [0]\n"
               "    --sin-strength <X> [0]  --sin-frequency <X> [1]                                  sine displacement\n"
               "    --mismatch-chance <X> [0]  --drop-features <X> [1]  --split-landmarks <X> [0]  --join-landmarks <X> [0]\n"
               "    --index-noise <host|device> [host]   where those four passes run: on the host arrays (sequential draws), or in\n"
               "                              place on the device-resident problem (counter-based draws: another result for a seed;\n"
               "                              one GPU only)\n"
               "    --seed <N>                every random draw is seeded (default: std::random_device)\n"
               "    --gpus <N> | --devices <a,b,...>   shard the problem over N GPUs of this node (contiguous camera ranges,\n"
               "                              points replicated, statistics and errors through RCCL); the same file for every N up to rounding\n";
    if (sub == "generate")
        return "city2ba generate <FILE.obj> <OUT>\n"
               "    --cameras <N> [100]   --points <N> [1000]   --max-dist <X> [100]\n"
               "    --intrinsics-start <f,k1,k2> [1,0,0]   --intrinsics-end <f,k1,k2> [1,0,0]\n"
               "    --path <NAME> [--step-size <X> [0]]    cameras along the polyline model NAME\n"
               "    --ground <X> [0]  --height <X> [1]     Poisson placement (without --path)\n"
               "    --move-to-origin   --no-lcc   --exact-lcc (extension)   --seed <N>\n";
    if (sub == "ply") return "city2ba ply <FILE> <OUT.ply>\n";
    if (sub == "covisibility")
        return "city2ba covisibility <FILE>\n"
               "    --min-shared <K> [1]      an edge joins two cameras that observe at least K points in common\n"
               "    prints the cameras, the edges, the maximum degree and the isolated cameras of that graph, built on the device\n";
    if (sub == "compare")
        return "city2ba compare <EST> <REF>\n"
               "    --on <cameras|points|both> [cameras]   what the similarity is fitted to: camera centres, points, or both pooled\n"
               "    --no-scale                the scale is held at 1\n"
               "    --max-dist <D>            trimming: after a fit only correspondences within D (in REF's frame) stay, and the fit is repeated\n"
               "    --rounds <N> [5]          ... at most N times (needs --max-dist); trimming starts from the least-squares fit, it is no\n"
               "                              consensus search: gross outliers can empty the set (status too_few)\n"
               "    --apply <OUT>             write EST moved into REF's frame\n"
               "    prints one JSON line: status, rounds, scale, rotation (row-major), translation, and per kind n, rmse, mean, max, argmax\n"
               "    (cameras: centre distance; camera_rotations_deg: angle to REF's rotation; points: distance), after the alignment\n";
    if (sub == "solve")
        return "city2ba solve <FILE> <OUT>\n"
               "    --iterations <N> [10]     --lambda <X> [1e-4]        Levenberg-Marquardt iterations, initial damping\n"
               "    --pcg-iterations <N> [100]  --pcg-tol <X> [1e-6]     the step's conjugate gradients\n"
               "    --function-tol <X> [0]  --gradient-tol <X> [0]  --parameter-tol <X> [0]   stopping tests (0: off)\n"
               "    --loss <squared|huber|cauchy|soft-l1> [squared]   --loss-scale <X> [1]\n"
               "    --preconditioner <block-jacobi|schur-jacobi> [block-jacobi]\n"
               "    --schur <implicit|explicit> [implicit]   explicit: the reduced camera system is formed once per step on the\n"
               "                              covisibility pattern and the conjugate gradients run on the stored blocks\n"
               "    --linear-solver <pcg|cholesky> [pcg]   cholesky: the reduced camera system is formed, factored densely on the\n"
               "                              device and solved exactly, without conjugate gradients (at most 4096 cameras)\n"
               "    --inner-iterations <N> [0] after every step, N rounds of per-point refinement of the points against the moved cameras,\n"
               "                              before the step's cost is taken (0: off)\n"
               "    --fix-intrinsics          hold f, k1, k2 of every camera constant\n"
               "    --fix-first-camera        hold the pose of camera 0 constant\n"
               "    --window <LO:HI>          solve cameras LO ... HI-1 and the points they see alone, with everything at the rim of the\n"
               "                              window held constant, and put the result back; the whole problem is written.  Every other\n"
               "                              flag applies to the window [off]\n"
               "    --no-halo                 with --window: take no cameras from outside the window; the points also seen from outside\n"
               "                              are held constant instead of the outside cameras that see the window's points\n"
               "    --window-around <C[,C...]>  the window is cameras C and the cameras that see what they see: those within --hops edges\n"
               "                              of the covisibility graph (cameras that share at least --min-shared points), at most\n"
               "                              --max-cameras of them, the nearest levels first and the last level by shared points;\n"
               "                              not with --window; --no-halo applies\n"
               "    --hops <N> [1]  --min-shared <K> [1]  --max-cameras <M> [no limit]\n"
               "    --filter-max-error <X>    outlier rejection: solve, drop the observations whose reprojection residual exceeds X,\n"
               "                              then solve again without a loss [off]\n"
               "    --filter-rounds <N> [1]   solve + filter rounds before the last solve\n"
               "    --filter-in-front         also drop observations whose point is not in front of its camera\n"
               "    --prior-from <FILE>       priors whose targets are FILE's camera centres, intrinsics and points (a .bal / .bbal with\n"
               "                              the same cameras; a point prior needs the same points); weight = 1 / sigma\n"
               "    --prior-center-sigma <S|SX,SY,SZ>            on every camera's centre\n"
               "    --prior-intrinsics-sigma <SF,SK1,SK2>        on every camera's f, k1, k2\n"
               "    --prior-point-sigma <S>  [--prior-point-every <N> [1]]   on every N-th point\n";
    if (sub == "triangulate")
        return "city2ba triangulate <FILE> <OUT>\n"
               "    --min-angle <DEG> [1]     parallax test: a point whose rays are less than DEG degrees apart keeps its position\n"
               "    --max-error <X>           consensus triangulation for a list with wrong matches: candidates from pairs of rays, the\n"
               "                              one most observations reproject within X of (in front of their cameras), a refit on those [off]\n"
               "    --min-inliers <N> [3]     a point whose best candidate has fewer inliers keeps its position (at least 2)\n"
               "    --max-hypotheses <H> [64] candidates per point, widest pairs first (1 ... 64)\n"
               "    --drop-outliers           then remove the observations of the triangulated points that are not inliers\n";
    if (sub == "resect")
        return "city2ba resect <FILE> <OUT>\n"
               "    --min-points <N> [6]      a camera with fewer usable observations keeps its pose (at least 6)\n"
               "    --min-gap <G> [1e-4]      degeneracy test: a camera whose points are so close to coplanar, or so little spread, that\n"
               "                              lambda_2 < G lambda_9 keeps its pose\n"
               "    --max-error <X>           consensus resection for a list with wrong matches: candidate poses from triples of\n"
               "                              observations, the one most observations reproject within X of (the point in front), the\n"
               "                              same fit on those [off]\n"
               "    --min-inliers <N> [6]     a camera whose best candidate has fewer inliers keeps its pose (at least 6; takes the\n"
               "                              place of --min-points)\n"
               "    --max-hypotheses <H> [64] candidates per camera, widest triples first (1 ... 64)\n"
               "    --drop-outliers           then remove the observations of the resected cameras that are not inliers\n";
    if (sub == "merge")
        return "city2ba merge <FILE> <OUT>\n"
               "    --radius <R>              two points at most R apart are candidates for one landmark (required)\n"
               "    --max-error <X>           they are merged when no camera sees both and every observation of both reprojects\n"
               "                              within X of the merged position, in front of its camera (required)\n"
               "    --rounds <N> [1]          rounds, each on the result of the last; a round that merges nothing is the last\n"
               "                              The absorbed points are not culled: they stay in the file as unobserved points.\n";
    if (sub == "rematch")
        return "city2ba rematch <FILE> <OUT>\n"
               "    --radius <R>              an observation that does not fit its point may take a point at most R from it, or a\n"
               "                              point that another such observation of the same camera gives up (required)\n"
               "    --max-error <X>           an observation fits a point when it reprojects within X of it, in front of its camera\n"
               "                              (required)\n"
               "    --min-fits <N> [2]        points that fewer than N observations fit are neither judged nor assigned\n"
               "                              An observation that fits no such point is removed.  Nothing is culled.\n";
    if (sub == "refine")
        return "city2ba refine <FILE> <OUT>\n"
               "    --rounds <N> [10]         rounds of per-point Levenberg-Marquardt: every point by itself, its own damping and acceptance,\n"
               "                              the cameras held (0: report only)\n"
               "    --lambda <L> [1e-4]       every point's initial damping\n"
               "    --loss <squared|huber|cauchy|soft-l1> [squared]   --loss-scale <A> [1]\n"
               "    --function-tol <T> [0]  --gradient-tol <T> [0]  --parameter-tol <T> [0]   per-point stopping tests (0: off)\n"
               "                              A point is written only when its cost fell.\n"
               "    --cameras                 refine every camera by itself instead, the points held (per-camera Levenberg-Marquardt: its own\n"
               "                              damping and acceptance; --rounds, --lambda and the stopping tests are then per camera)\n"
               "    --alternate <N>           N sweeps of both: every camera, then every point, with the options above for each\n";
    return nullptr;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2 || !std::strcmp(argv[1], "--help") || !std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "help")) {
        usage();
        return argc < 2 ? 1 : 0;
    }
    const std::string sub = argv[1];
    c2b_host_set_io_threads(env_int("C2B_IO_THREADS", 0));               // the handle-less host entries (c2b_bal_read / _write)
    for (int k = 2; k < argc; ++k)
        if (!std::strcmp(argv[k], "--help") || !std::strcmp(argv[k], "-h")) {
            const char *h = subcommand_help(sub);
            if (h) { std::printf("%s    --device <N>              GPU index [0]; C2B_TIMING=1 prints phase times\n", h); return 0; }
        }
    if (sub == "synthetic") return run_synthetic(argc, argv);
    if (sub == "synthetic-line") return run_synthetic_line(argc, argv);
    if (sub == "noise") return run_noise(argc, argv);
    if (sub == "generate") return run_generate(argc, argv);
    if (sub == "ply") return run_ply(argc, argv);
    if (sub == "solve") return run_solve(argc, argv);
    if (sub == "covisibility") return run_covisibility(argc, argv);
    if (sub == "compare") return run_compare(argc, argv);
    if (sub == "triangulate") return run_triangulate(argc, argv);
    if (sub == "resect") return run_resect(argc, argv);
    if (sub == "merge") return run_merge(argc, argv);
    if (sub == "rematch") return run_rematch(argc, argv);
    if (sub == "refine") return run_refine(argc, argv);
    die("The subcommand '" + sub + "' wasn't recognized");
}
