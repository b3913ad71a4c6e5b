// C ABI of the MI355X EqF hot path (include/eqf_vio_amd.h): handle management, host-side landmark
// bookkeeping (integer id matching, eqf_vio/src/VIOFilter.cpp:211-230, :345-443) and kernel launches.
// All arithmetic of the filter runs in the HIP kernels of eqf_propagate.hpp / eqf_update.hpp /
// eqf_churn.hpp; there is no CPU fallback: without a usable GPU eqf_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/eqf_vio_amd_debug.h"  // (the public header + the test / measurement hooks this library also exports)
#include "eqf_churn.hpp"
#include "eqf_dense.hpp"
#include "eqf_device.hpp"
#include "eqf_propagate.hpp"
#include "eqf_burst.hpp"
#include "eqf_chol64.hpp"
#include "eqf_resident.hpp"
#include "eqf_update.hpp"
#include "eqf_i8.hpp"
#include "eqf_local.hpp"
#include "eqf_innov.hpp"
#include "eqf_factor.hpp"
#include "eqf_nees.hpp"
#include "eqf_clone.hpp"
#include "eqf_clone_host.hpp"
#include "eqf_frame.hpp"
#include "eqf_sample.hpp"
#include "eqf_sample_host.hpp"
#include "eqf_blocks.hpp"
#include "eqf_blocks_host.hpp"
#include "eqf_linear.hpp"
#include "eqf_linear_host.hpp"
#include "eqf_mixture.hpp"
#include "eqf_mixture_host.hpp"
#include "eqf_mergecost.hpp"
#include "eqf_mergecost_host.hpp"
#include "eqf_forecast.hpp"
#include "eqf_forecast_host.hpp"
#include "eqf_score.hpp"
#include "eqf_score_host.hpp"
#include "eqf_lift.hpp"
#include "eqf_lift_host.hpp"
#include "eqf_border_host.hpp"
#include "eqf_mapedit.hpp"
#include "eqf_mapedit_host.hpp"
#include "eqf_iterate.hpp"
#include "eqf_observe.hpp"
#include "eqf_schmidt.hpp"
#include "eqf_schmidt_host.hpp"
#include "eqf_split.hpp"
#include "eqf_split_host.hpp"
#include "eqf_workspace.hpp"

using namespace eqf;

#define HIPC(expr)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            std::fprintf(stderr, "eqf_vio_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return EQF_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

namespace {
constexpr int kRing = 64;

struct ProfPair {
    int cls, key;
    hipEvent_t a, b;
};
struct ProfSample {
    int key;  // launch shape within the class (chain step index, burst length, ...): launches of one key do identical work
    float ms;
};

// the downdate on the integer pipe (eqf_i8.hpp).  u != nullptr: the innovation lift rides along in the split launch (the per-column launch
// shapes; k_chol_resident ran it in its roles)
void launchI8Dd(int slices, const I8DdArgs& a, const UpdArgs* u, int nCt, hipStream_t st) {
    UpdArgs uu{};
    if (u) uu = *u;
    i8WithSlices(slices, [&](auto s) {
        hipLaunchKernelGGL((k_i8dd_split<s>), dim3(nCt + (u ? 1 : 0), a.B), dim3(256), 0, st, a, uu, u ? 1 : 0);
        hipLaunchKernelGGL((k_i8dd_syrk<s>), dim3(a.nt * (a.nt + 1) / 2 * a.B), dim3(256), kI8ddLdsBytes, st, a);
    });
}
}  // namespace

// Ring of pinned int buffers for the small host->device uploads of the landmark bookkeeping (permutation, compaction map,
// sources of new landmarks): the host never has to drain the stream before reusing a staging buffer.
struct IntStage {
    static constexpr int kSlots = 8;
    PinnedPtr<int> host[kSlots];
    Event ev[kSlots];
    int next = 0;
};

// ---- What the optional routes keep on the handle: one sub-struct per route -- owners, capacities, the flag "dynamic-LDS attributes set"
// and options --, all of them behind the members the per-step calls touch (see the end of eqf_filter).  A route states its sizes where it
// reserves (reserveSlots); nothing here is freed by hand.
// joint NEES / log det (eqf_nees.hpp; eqf_get_nees): error vectors -> z [B][kNeesRhs][ld], the record of the current diagonal block
// [B][kDRec], the results [B][kNeesHead + kNeesRhs], and the pivot words [B]
struct NeesRoute {
    DevPtr<double> E, D, out;
    DevPtr<int> bad;
    bool ldsSet = false;
};
// draws from the covariance (eqf_sample.hpp; eqf_sample_sigma / eqf_apply_increment / eqf_perturb_filters): the samples and their images
// [B][rows][ld] (cap: bytes of each); and the small operands of a call that does not wait for the device -- scale [B] | vectors
// [B][kLm0 + 3 cap] (z of a perturbation or the increments) | mask [B] bytes -- as a staged image
struct SampRoute {
    DevPtr<double> Z, E;
    size_t cap = 0;
    StagedImage<> small;
};
// the low-rank linear measurement update (eqf_linear.hpp; eqf_update_linear): the operands of a call as a staged image
// (linear::SmallLayout), the workspace [B][linear::WorkLayout::stride()] and the result records [B][kLinHead]
struct LinRoute {
    StagedImage<> small;
    DevPtr<double> ws, out;
};
// the per-landmark block measurement update (eqf_blocks.hpp; eqf_update_landmarks), grown when a call's stride or rows ask for more: the
// operands of a call as a staged image (blocks::SmallLayout), the workspace in doubles and in ints (blocks::WorkLayout; capacities in
// bytes), the records [B][kLinHead] and, from the first eqf_observe_landmarks, the rows that call forms (observe::RowsLayout; capacity in
// bytes)
struct BlkRoute {
    StagedImage<> small;
    DevPtr<double> ws, out, obs;
    DevPtr<int> wi;
    size_t wsCap = 0, wiCap = 0, obsCap = 0;
    bool ldsSet = false, downLdsSet = false;  // (the factorisation's kernels; k_blk_downdate)
};
// the innovation lift of eqf_update_linear / eqf_update_landmarks / eqf_apply_increment / eqf_perturb_filters (eqf_lift.hpp;
// eqf_set_option "innovation_lift"): the records [B][kLiftRec] of the last of these calls, and -- from the first call with the option on
// -- the right-hand-side rows [B][kLiftRhs][ld], the record of the current diagonal block [B][kDRec] and the pivot words [B] (the image
// that is factored is dSigmaLoc)
struct LiftRoute {
    int opt = 0;
    bool called = false, ldsSet = false;
    DevPtr<double> rec, E, D;
    DevPtr<int> bad;
};
// eqf_copy_filters (eqf_clone.hpp): the pair table (pinned image + device copy, grown on demand; pairsCap in bytes), the small-state
// staging image of the in-place case and two events -- evSrc orders a copy behind this handle's work when it is the source, evDone marks
// the end of the last copy INTO this handle (its pair table may be reused, the source may go on)
struct CloneRoute {
    PinnedPtr<ClonePair> hPairs;
    DevPtr<ClonePair> dPairs;
    size_t pairsCap = 0;
    DevPtr<char> small;
    Event evSrc, evDone;
};
// moment matching over the handle's filters (eqf_mixture.hpp; eqf_get_mixture_moments / eqf_merge_filters): the workspace
// (mixture::WorkLayout) and the member table of a call as a staged image, grown on demand (members, then the distinct filters)
struct MixRoute {
    DevPtr<double> ws;
    StagedImage<> tab;
    int launches = 0;  // kernel launches of the most recent mixture call, counted as they are made (eqf_debug_mixture_launches)
};
// the non-mutating forecast (eqf_forecast.hpp; eqf_forecast): the samples of a call as a pinned image and its device copy, the per-step
// records the builder leaves for the landmark lanes, and the output records as a device image and its pinned copy
// (forecast::imageCapacityDoubles / recDoubles / outStride).  The call synchronises before it returns, so the pinned images need no event.
struct ForecastRoute {
    PinnedPtr<ImuRec> hImu;
    DevPtr<ImuRec> dImu;
    DevPtr<double> rec, dOut;
    PinnedPtr<double> hOut;
};
// pairwise merge costs (eqf_mergecost.hpp; eqf_get_merge_costs): one block for a chunk of images with their right-hand sides, records
// and orders (grown when the option "merge_cost_chunk" asks for more), one for a call's items and records
struct MergeCostRoute {
    DevPtr<char> ws, items;
    size_t wsBytes = 0, itemBytes = 0;
    int chunkCap = 0, chunkOpt = 0;  // (what the blocks were carved for)
    size_t itemCap = 0;
};
// scoring candidate frames (eqf_score.hpp; eqf_score_vision): one block for a chunk of images of order score::paddedOrder(capacity) with
// their right-hand-side rows, diagonal-block records and pivot words (grown when the option "score_chunk" asks for more), one for a
// call's items, matched slots, bearings, per-landmark statistics and records
struct ScoreRoute {
    DevPtr<char> ws, tab;
    size_t wsBytes = 0, tabBytes = 0;
    int chunkCap = 0, chunkOpt = 0;
    bool ldsSet = false;
};
// explicit landmark edits (eqf_mapedit.hpp; eqf_edit_landmarks): the plan's image (mapedit::Image) as a staged image
struct MapEditRoute {
    StagedImage<> img;
};
// the Schmidt updates (eqf_schmidt.hpp; eqf_update_linear_schmidt / eqf_update_landmarks_schmidt): the partition's image
// (schmidt::Image) as a staged image whose pinned side k_schmidt_gamma reads through its device-side address
struct SchmidtRoute {
    StagedImage<true> img;
    bool ldsSet = false;
};
// eqf_split_filters (eqf_split.hpp): the plan's image (split::Image: rows, shifts, shrinks, the source, child and pair tables) as a
// staged image, and the workspace (split::Work: Ht, B, u, the increments, the verdict records and the increment step's mask)
struct SplitRoute {
    StagedImage<> img;
    DevPtr<char> ws;
};
// the iterated landmark observation update (eqf_iterate.hpp; eqf_observe_landmarks_iterated), grown when a call asks for more: the
// workspace in doubles [B][iterate::WorkLayout::strideD()] and in ints [B][kInts], g_trace on the device (iterate::traceDoubles); capacities
// in bytes.  The two row buffers are BlkRoute::obs at twice its size.  launches: the kernel launches the most recent such call added to
// eqf_observe_landmarks's own, counted as they were made (eqf_debug_iterate_launches).
struct IterRoute {
    DevPtr<double> ws, trace;
    DevPtr<int> wi;
    size_t wsCap = 0, traceCap = 0, wiCap = 0;
    bool ldsSet = false;
    int launches = 0;
};

struct eqf_filter {
    int B = 0, cap = 0, device = 0, precision = 0;
    size_t esz = 8;
    eqf_settings set{};
    Params prm{};
    Stream stream;  // (in front of every buffer and event: members go in reverse order, the stream last)
    int nTot = 0, ld = 0;
    long long sigmaStride = 0;
    DevPtr<void> Sigma[2];
    DevPtr<Glob> g[2];
    DevPtr<double> p0;
    DevPtr<double> lmc;  // [B][15][cap] per-landmark constants (C0i, chart rotation)
    DevPtr<double> Q[2];
    int pS = 0, pG = 0;
    // update chains
    DevPtr<double> SA, SL, YW, YO, EA, EL, ZW, ZO;
    int ldS = 0, ldY = 0, ldE = 0, ldZ = kSB;
    long long strideDS = 0, strideDE = 0;  // diagonal-factor records of the two chains
    long long strideS = 0, strideY = 0, strideE = 0, strideZ = 0;
    DevPtr<double> dbgDelta, dbgGamma, dbgGammaTot, red;
    DevPtr<int> errflag;
    // churn scratch
    DevPtr<int> dMap;
    int* dNewN = nullptr;  // (= dMap + B * cap)
    DevPtr<int> dPerm;
    std::vector<std::vector<int>> permOnDevice;  // what dPerm holds (uploadPerm): the same landmark set in the same order needs no new copy
    DevPtr<double> dChord, dDepth2, dScratch, dMeas, dOut;
    IntStage stMap, stPerm;  // pinned rings: [B*cap + B] (map + new counts), [B*cap]
    IntStage stEdit;         // pinned ring [frame::ImageLayout::editInts()]: keep map | permutation | counts of a k_edit launch (one upload per frame)
    DevPtr<int> dEdit;       // its device image
    std::vector<int> editOnDevice;  // ... as last uploaded
    DevPtr<int> dEditBar;    // [B][4] k_edit's counters
    int lastBurstShape[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // eqf_debug_launch_shape: the most recent IMU burst's launch shape
    std::vector<char> restoredMark; // [B] eqf_set_state since the last reset: once every filter has been restored a hand-off time-out (bit 128) is forgiven
    // OCC2 grids from this many roles per CU on read the E-chain's tiles in Sigma itself instead of a copy made by the prep launch
    // (eqf_debug_option "e_sigma_min_percu_x10").  8.0 until late round 5 ("at 8 filters of N = 200, 6.3 roles per CU, the kernel loses what
    // the prep launch gains"); measured again behind the gated downdate: 8 filters 323.5 -> 331.3 k steps/s (prep 29.6 -> 19.2 us, kernel
    // 158.9 -> 164.1), 10 filters 345.7 -> 354.3 k; 5 / 6 / 7 filters 232.0 -> 232.9 k, 259.6 -> 262.1 k, 292.1 -> 296.8 k: every grid of the
    // two-per-CU build (chain roles per CU: 0.57 per filter of N = 200; profiles/r05_e_sigma_threshold.txt)
    double eSigmaMinPerCU = 2.4;
    // the fused burst launch up to this many workgroups per CU (eqf_debug_option "burst_fused_max_x10").  It cannot deadlock on any grid (builders
    // first, and they wait for nobody), but its bodies are the latency ones -- 4-landmark builders, one row per wavefront, 512 threads:
    // measured at N = 200 (profiles/r05_fused_oversub.txt, steps/s, two launches -> fused): 2 filters (1.2 per CU) 120.3 -> 122.3 k; 3 filters
    // (1.8) 167.7 -> 160.0 k; 4: 214.8 -> 192.9 k; 8: 331 -> 266 k.  A fused launch for batches would need the throughput bodies (16-landmark
    // builders, two / four rows per wavefront) with the flag protocol: sized at 27 us of a 262 us frame at 8 filters, not built.
    double fusedMaxPerCU = 1.25;
    int deviceEdit = 1;      // landmark-set changes and the outlier gate of a frame in ONE launch, decided on the device (eqf_debug_option "device_edit")
    DevPtr<double> dDepthSel;    // [B] median scene depth selected on the device
    PinnedPtr<double, true> hChord;  // (with its device-side address: hChord.dev)
    PinnedPtr<double> hMeas, hOut;
    Event evMeas;
    bool measPending = false;    // eqf_process_vision: the bearings sit in hMeas, their copy is visionCore's to enqueue (with k_edit's image behind them)
    // input ring for per-call records (batch > 1)
    DevPtr<ImuRec> dRing;
    PinnedPtr<ImuRec> hRing;
    Event evRing[kRing];
    bool ringUsed[kRing] = {};
    long long ringCount = 0;
    // stream mode
    DevPtr<ImuRec> sImu;   // [K][B]
    DevPtr<ImuRec> sVis;   // [F][B] (stamp only)
    DevPtr<double> sBear;  // [F][B][nb][3]
    int sK = 0, sF = 0, sNb = 0;
    std::vector<int> sIds;
    std::vector<double> hImuStamp, hVisStamp;  // host mirrors of the stamps
    // host mirrors
    std::vector<std::vector<int>> ids;
    std::vector<double> curTime;
    std::vector<char> init;
    std::vector<char> devInit;  // the filter's lazy initialisation has been LAUNCHED (init is set when the call is queued)
    int densePropagate = 0;
    DevPtr<void> dF, dG, dBn;  // dense backend: F, G = F Sigma, Bn (n x 6)
    DevPtr<void> dBlk;         // split propagate path: per-landmark records [B][cap][kBlkRec] (T)
    DevPtr<CommonLds> dBlkCommon;
    int splitPropagate = -1;       // -1 heuristic, 0 never, 1 always (EQF_SPLIT_PROPAGATE)
    bool ldsAttrSet = false;       // hipFuncAttributeMaxDynamicSharedMemorySize applied on this handle's device (allowUpdateLds)
    // speculative outlier gate: the frame whose gate answer the host has not looked at yet
    struct {
        bool pending = false;
        std::vector<std::vector<int>> ids;  // measurement ids per filter
        std::vector<int> nb;
        std::vector<char> active;
        std::vector<int> nOld;              // landmarks per filter before the frame's new ones were appended
        const double* bearings = nullptr;   // device
        long long bearStride = 0;
        bool onDevice = false;              // k_edit removed the outliers itself: only the host's id lists are left to bring up to date
        std::vector<int> nKept;             // ... kept landmarks per filter (the chords in hChord are in that order)
    } gate;
    PinnedPtr<int, true> hGate;  // pinned [B]: raised by k_probe (with its device-side address: hGate.dev)
    DevPtr<int> dMask;           // [B]
    Event evGate;
    Event evMask;                  // k_set_update_ok has read hGate (resolveGate's redo): recorded before the host may clear it again
    bool maskPending = false;
    int csInBurst = 1;           // bursts closed by a vision step also leave C Sigma' and S (BurstArgs::csOut; eqf_debug_option "cs_in_burst")
    bool csValid = false;        // ... and they are still what the update would compute (nothing moved a landmark since)
    int gateSpeculative = 1;     // EQF_GATE_SPECULATIVE = 0: always wait for the gate's answer before the update
    // the outlier gate of the handle (eqf_set_outlier_gate): what is compared -- the chord or the Mahalanobis distance -- and with what.
    // eqf_create sets (EQF_GATE_CHORD, settings.outlierThreshold); a setting, not state: eqf_reset / eqf_set_state / eqf_copy_filters leave it
    int gateKind = EQF_GATE_CHORD;
    double gateThr = 0.0;
    // eqf_get_gate_report: what the gate of the most recent vision call looked at, per filter, in the state's order before the removals --
    // taken from the pinned hChord where the host applies the device's decision (recordGate); empty: not examined
    struct GateReport {
        std::vector<int> ids;
        std::vector<double> stat;
        std::vector<char> removed;
    };
    std::vector<GateReport> report;
    // IMU bursts (eqf_burst.hpp): processIMUData calls are queued on the host and launched together -- when the queue is
    // full, when the vision call that follows them arrives (whose integrateUpToTime joins the burst), or when the host
    // touches the handle in any other way.  burstMax = 0: every call launches at once through k_propagate.
    int burstMax = kBurstMax;      // EQF_IMU_BURST / eqf_set_imu_burst
    int burstRows = 0;             // block kernel: row landmarks per wavefront, 0 = by launch size (EQF_BURST_ROWS = 1 | 2 | 4)
    int ringAhead2 = 0;            // block kernel with two row landmarks per wave: constants requested two steps ahead -- measured 1.5-2.7 us SLOWER per burst at 4..12 filters (profiles/r06_burst_shapes.txt), kept behind eqf_debug_option "ring_ahead2"
    int burstLm = 0;               // builder: landmarks per workgroup, 0 = by launch size (eqf_debug_option "burst_lm")
    struct {
        int kind = 0;              // 0 nothing pending, 1 records k0 .. k0+cnt-1 of the uploaded stream, 2 inline records (one filter)
        int k0 = 0, cnt = 0;
        ImuRec inl[kBurstMax];
    } burst;
    DevPtr<void> dColRec, dRowRec;  // per step and landmark records of k_burst_build
    DevPtr<BurstStep> dSteps;
    int cholSplit = -1;            // -1 heuristic, 0 fused chain launches, 1 panel + update launches (EQF_CHOL_SPLIT)
    DevPtr<int> dFlags;            // [B][2][flagStride]: epoch flags of the in-launch hand-off of the diagonal-factor records
    int flagStride = 0;
    int updateEpoch = 0;           // one per launchUpdate
    // k_chol_resident (one launch per update while the grid fits the chip): EQF_CHOL_RESIDENT = 0 switches it off
    int cholResident = 1;
    int resFoldPrep = 1;           // co-resident grid: the prep work as roles of the SAME launch (EQF_RES_FOLD_PREP = 0: k_update_prep64 launched first)
    DevPtr<int> dPrepFlags;        // [B][nPrepCap]
    int nPrepCap = 0;
    int burstFused = 1;            // latency case: builder and block workgroups of a burst in ONE launch (EQF_BURST_FUSED = 0: two launches)
    DevPtr<int> dBuildFlags;       // [B][nBuildCap]: steps each builder workgroup has published, + 32 * burstEpoch
    int nBuildCap = 0, burstEpoch = 0;
    int residentPerCU = -1;        // hipOccupancyMaxActiveBlocksPerMultiprocessor of k_chol_resident on this device (lazily queried)
    int numCUs = 0;
    int nbCap = 0, wtCap = 0;
    DevPtr<int> dReadyA, dReadyY, dResCounters, dStageFlags;
    DevPtr<unsigned> dTicket;     // k_chol_resident on a grid larger than the chip: arrival tickets, [B][32] (ResArgs::ticket); ticketBase = tickets drawn per filter by earlier launches
    unsigned ticketBase = 0;
    // the covariance downdate on the integer matrix pipe (eqf_i8.hpp; eqf_set_option "downdate_slices"): slices (0 = fp64), and the
    // workspace of the split -- slices for i8Slices, i8WsStride bytes per filter (i8WsBytes in all), and the columns' exponent words
    int ddSlices = 0, i8Slices = 0;
    DevPtr<signed char> dI8Ws;
    DevPtr<int> dI8Expo;
    long long i8WsStride = 0;
    size_t i8WsBytes = 0;
    // covariance in the coordinates of the estimate (eqf_local.hpp): the J blocks [B][kJacHead + 9 cap] and an image of Sigma's size, both
    // allocated by the first call that needs them.  dSigmaLoc is ONE slot that the getters, NEES and the draws, the lift, the mixture
    // routes and the in-place copy all name (sigmaLocWant)
    DevPtr<double> dJac, dSigmaLoc;
    // innovation statistics of every update (eqf_innov.hpp; eqf_set_option "innovation_stats"): the tail launch k_innov_stats and its
    // records [B][kInnovHead + cap], allocated when the option is first switched on
    int innovStats = 0;
    DevPtr<double> dInnov;
    int resTickets = 0;           // eqf_debug_option "res_tickets": 0 (default) the block index (rounds 3-5), 1 tickets on grids >= 6 x the resident slots, 2 on every grid larger than the chip (non-FOLD)
    DevPtr<double> dGammaPart, dG11Part;
    DevPtr<ResRole> dRoles;
    size_t rolesBytes = 0;            // (capacity of dRoles)
    int rolesN = -1, rolesCount = 0;  // chain shape (nbS, nbE, wtS) the role table was built for
    unsigned long long rolesOmit = 0; // ... and the right-hand-side roles W(0, C) of the E-chain it leaves out (bit C; border rows)
    int resBorder = 1;                // eqf_debug_option "res_border": the co-resident update launch carries the lift's regressors as border rows of the E-chain's last block row (eqf_border_host.hpp); 0: the right-hand-side roles of the E-chain as before
    bool countsExact = true;          // the landmark counts the update will find on the device are the host's (false: a device-side outlier gate may lower them)
    int rolesFront = 0;               // roles in front of the prep roles (buildRoles' `front`)
    int dropRole[4] = {-1, 0, 0, 0};  // eqf_debug_drop_role: (kind, role, R, C) of the role whose workgroup leaves without publishing anything
    // profiling (the event pool is the one place that creates and destroys events by hand)
    bool prof = false;
    std::vector<ProfPair> profPairs;
    std::vector<hipEvent_t> evPool;
    long long profCount[EQF_PROF_CLASSES] = {};
    double profMs[EQF_PROF_CLASSES] = {};
    std::vector<ProfSample> profSamples[EQF_PROF_CLASSES];  // per-bracket times with their launch shape
    double profOverheadMs = 0.0;  // elapsed time of an EMPTY event bracket (calibrated when profiling is switched on)
    // ---- the optional routes, behind everything the per-step calls touch (R21.1: a route's pointers in the middle of the handle cost
    // 0.6 % of the benchmark).  A new route adds a sub-struct here and names its slots where it reserves.
    NeesRoute nees;
    SampRoute samp;
    LinRoute lin;
    BlkRoute blk;
    LiftRoute lift;
    CloneRoute clone;
    MixRoute mix;
    ForecastRoute fc;
    MergeCostRoute mc;
    ScoreRoute sc;
    MapEditRoute medit;
    SchmidtRoute sch;
    SplitRoute split;
    IterRoute iter;

    ~eqf_filter() {
        for (auto e : evPool) (void)hipEventDestroy(e);
        for (auto& p : profPairs) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    }
};

namespace {

template <typename F>
int profiled(eqf_filter* f, int cls, F&& launch, int key = 0) {
    if (!f->prof) {
        launch();
        return EQF_OK;
    }
    hipEvent_t a, b;
    for (hipEvent_t* e : {&a, &b}) {
        if (!f->evPool.empty()) {
            *e = f->evPool.back();
            f->evPool.pop_back();
        } else {
            HIPC(hipEventCreate(e));
        }
    }
    HIPC(hipEventRecord(a, f->stream));
    launch();
    HIPC(hipEventRecord(b, f->stream));
    f->profPairs.push_back({cls, key, a, b});
    return EQF_OK;
}

int profDrain(eqf_filter* f) {
    HIPC(hipStreamSynchronize(f->stream));
    for (auto& p : f->profPairs) {
        float ms = 0;
        HIPC(hipEventElapsedTime(&ms, p.a, p.b));
        f->profCount[p.cls]++;
        f->profMs[p.cls] += ms;
        f->profSamples[p.cls].push_back({p.key, ms});
        f->evPool.push_back(p.a);
        f->evPool.push_back(p.b);
    }
    f->profPairs.clear();
    return EQF_OK;
}

// `count` elements (of `esz` bytes where the owner is untyped) into an owner; what it held is freed first
template <typename T>
int dmalloc(DevPtr<T>& p, size_t count, size_t esz = sizeof(std::conditional_t<std::is_void<T>::value, char, T>)) {
    p.reset();
    HIPC(hipMalloc(p.slot(), std::max<size_t>(count, 1) * esz));
    return EQF_OK;
}
template <typename T, bool M>
int hmalloc(PinnedPtr<T, M>& p, size_t count) {
    p.reset();
    HIPC(hipHostMalloc(p.slot(), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
    if constexpr (M) HIPC(hipHostGetDevicePointer(p.mapped(), p.get(), 0));
    return EQF_OK;
}

// ---- the HIP side of the allocation transaction (eqf_workspace_host.hpp)
struct HipBackend {
    hipStream_t stream;
    void* allocDevice(size_t bytes) {
        void* p = nullptr;
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    void* allocPinned(size_t bytes, void** mapped) {
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        if (mapped && hipHostGetDevicePointer(mapped, p, 0) != hipSuccess) {
            (void)hipHostFree(p);
            return nullptr;
        }
        return p;
    }
    void* allocEvent() {
        hipEvent_t e = nullptr;
        return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? e : nullptr;
    }
    void freeDevice(void* p) { (void)hipFree(p); }
    void freePinned(void* p) { (void)hipHostFree(p); }
    void freeEvent(void* p) { (void)hipEventDestroy(static_cast<hipEvent_t>(p)); }
    bool drain() { return hipStreamSynchronize(stream) == hipSuccess; }
    void clearError() { (void)hipGetLastError(); }  // (a failed allocation must not fail the next launch through the sticky last error)
};
// the wants of the owners
template <class T>
workspace::Want want(DevPtr<T>& p, size_t bytes, size_t* cap = nullptr) { return workspace::device(p.slot(), bytes, cap); }
template <class T>
workspace::Want want(PinnedPtr<T, false>& p, size_t bytes, size_t* cap = nullptr) { return workspace::pinned(p.slot(), bytes, cap); }
template <class T>
workspace::Want want(PinnedPtr<T, true>& p, size_t bytes, size_t* cap = nullptr) { return workspace::pinned(p.slot(), bytes, cap, p.mapped()); }
inline workspace::Want want(Event& e) { return workspace::event(e.slot()); }
// (a staged image is three wants: WANT_STAGED(image, bytes) inside a list)
#define WANT_STAGED(im, bytes) want((im).host, (bytes), &(im).cap), want((im).dev, (bytes), &(im).cap), want((im).read)
// Everything a call needs, all or nothing (workspace::reserve): EQF_ERR_HIP leaves the handle exactly as it was.  `installed`: which
// wants this call allocated.
template <int N>
int reserveSlots(eqf_filter* f, const workspace::Want (&w)[N], workspace::Result* installed = nullptr) {
    HipBackend be{f->stream};
    const workspace::Result r = workspace::reserve(be, w);
    if (installed) *installed = r;
    return r.ok ? EQF_OK : EQF_ERR_HIP;
}
// the image of Sigma's size that several routes share: one slot
workspace::Want sigmaLocWant(eqf_filter* f, bool wanted = true) {
    return want(f->dSigmaLoc, wanted ? sizeof(double) * size_t(f->sigmaStride) * f->B : 0);
}

int eventInit(eqf_filter* f, Event& e) {
    const workspace::Want w[] = {want(e)};
    return reserveSlots(f, w);
}
int stageInit(eqf_filter* f, IntStage& s, size_t count) {
    for (int i = 0; i < IntStage::kSlots; ++i) {
        int rc = hmalloc(s.host[i], count);
        if (!rc) rc = eventInit(f, s.ev[i]);
        if (rc) return rc;
    }
    return EQF_OK;
}
// next free staging buffer (waits only if its previous upload, 8 uploads ago, is still in flight)
int stageAcquire(IntStage& s, int** host, int* slot) {
    *slot = s.next;
    s.next = (s.next + 1) % IntStage::kSlots;
    HIPC(hipEventSynchronize(s.ev[*slot]));
    *host = s.host[*slot];
    return EQF_OK;
}

// VIOFilter(const Settings&) initial values (VIOFilter.cpp:60-73, VIOFilter.h:45-55)
int initState(eqf_filter* f) {
    const int B = f->B;
    std::vector<Glob> g0(B);
    for (auto& g : g0) {
        std::memset(&g, 0, sizeof(Glob));
        g.P0q[0] = 1.0;
        g.Aq[0] = 1.0;
        for (int i = 0; i < 3; ++i) {
            g.bias[i] = f->set.initialOmegaBias[i];
            g.bias[3 + i] = f->set.initialAccelBias[i];
        }
        g.curTime = -1.0;
    }
    for (int p = 0; p < 2; ++p) {
        HIPC(hipMemcpyAsync(f->g[p], g0.data(), sizeof(Glob) * B, hipMemcpyHostToDevice, f->stream));
        HIPC(hipMemsetAsync(f->Sigma[p], 0, f->esz * f->sigmaStride * B, f->stream));
        HIPC(hipMemsetAsync(f->Q[p], 0, sizeof(double) * 5 * f->cap * B, f->stream));
    }
    HIPC(hipMemsetAsync(f->p0, 0, sizeof(double) * 3 * f->cap * B, f->stream));
    HIPC(hipMemsetAsync(f->errflag, 0, sizeof(int), f->stream));
    if (f->dEditBar) HIPC(hipMemsetAsync(f->dEditBar, 0, sizeof(int) * 4 * B, f->stream));  // (k_edit's counters: a launch that timed out leaves them mid-count)
    // Sigma base block diag
    std::vector<double> base(12 * 12, 0.0);
    for (int i = 0; i < 3; ++i) {
        base[i * 12 + i] = f->set.initialBiasOmegaVariance;
        base[(3 + i) * 12 + 3 + i] = f->set.initialBiasAccelVariance;
        base[(8 + i) * 12 + 8 + i] = f->set.initialVelocityVariance;
    }
    base[6 * 12 + 6] = base[7 * 12 + 7] = f->set.initialGravityVariance;
    std::vector<float> basef(base.begin(), base.end());
    for (int b = 0; b < B; ++b) {
        char* dst = static_cast<char*>(f->Sigma[0]) + f->esz * f->sigmaStride * b;
        const void* src = f->precision == EQF_PRECISION_F32 ? static_cast<const void*>(basef.data()) : static_cast<const void*>(base.data());
        HIPC(hipMemcpy2DAsync(dst, f->esz * f->ld, src, f->esz * 12, f->esz * 12, 12, hipMemcpyHostToDevice, f->stream));
    }
    HIPC(hipStreamSynchronize(f->stream));
    f->pS = f->pG = 0;
    f->gate.pending = false;
    f->measPending = false;
    f->csValid = false;
    f->editOnDevice.clear();
    f->ids.assign(B, {});
    f->report.assign(B, {});
    f->curTime.assign(B, -1.0);
    f->init.assign(B, 0);
    f->devInit.assign(B, 0);
    return EQF_OK;
}

int resolveGate(eqf_filter* f);
int flushBurst(eqf_filter* f);
// Every entry point that looks at (or changes) the filter first settles what the host has deferred: the speculative gate
// of the last vision frame, then the queued IMU steps (in this order: they come after that frame).
#define GATE(f)                                                        \
    do {                                                               \
        if (hipSetDevice((f)->device) != hipSuccess) return EQF_ERR_HIP; \
        int grc_ = resolveGate(f);                                     \
        if (!grc_) grc_ = flushBurst(f);                               \
        if (grc_) return grc_;                                         \
    } while (0)

int maxN(const eqf_filter* f) {
    size_t m = 0;
    for (auto& v : f->ids) m = std::max(m, v.size());
    return int(m);
}
// the layouts that follow from batch and capacity alone: the frame's pinned image, the small state (its arrays and their staging image)
frame::ImageLayout frameImage(const eqf_filter* f) { return {size_t(f->B), size_t(f->cap)}; }
clone::SmallLayout cloneSmall(const eqf_filter* f) { return {size_t(f->B), size_t(f->cap), sizeof(Glob), size_t(kInnovHead)}; }
std::vector<int> landmarkCounts(const eqf_filter* f) {
    std::vector<int> N(f->ids.size());
    for (size_t b = 0; b < N.size(); ++b) N[b] = int(f->ids[b].size());
    return N;
}

// ---- the host's mirror of a filter (ids, clock, the two initialisation flags, the gate report) where a call makes filter d a copy of s
struct Mirror {
    std::vector<int> ids;
    double curTime;
    char init, devInit;
};
Mirror mirrorOf(const eqf_filter* f, int s) { return Mirror{f->ids[s], f->curTime[s], f->init[s], f->devInit[s]}; }
// dst's filter d takes over a mirror (of src's filter s); its gate report starts over (the gate and its threshold are settings: they stay)
void adoptMirror(eqf_filter* dst, int d, Mirror m) {
    dst->ids[d] = std::move(m.ids); dst->curTime[d] = m.curTime; dst->init[d] = m.init; dst->devInit[d] = m.devInit;
    dst->report[d] = {};
}
void adoptMirror(eqf_filter* dst, int d, const eqf_filter* src, int s) { adoptMirror(dst, d, mirrorOf(src, s)); }
// Would adoptMirror(f, d, f, s) change nothing?  (Then a call need not wait for the device's verdict to know the mirror of d.)
bool mirrorsAgree(const eqf_filter* f, int d, int s) {
    return f->ids[d] == f->ids[s] && f->curTime[d] == f->curTime[s] && f->init[d] == f->init[s] && f->devInit[d] == f->devInit[s] &&
           f->report[d].ids.empty();
}
// what the host caches about the device's Sigma and landmark sets starts over
void forgetDeviceCaches(eqf_filter* f) {
    f->csValid = false;
    f->permOnDevice.clear();
    f->editOnDevice.clear();
}

// Can the handle's gate remove anything?  A chord between unit vectors never exceeds 2; a Mahalanobis distance is finite.
bool gateCanTrip(const eqf_filter* f) { return f->gateKind == EQF_GATE_MAHALANOBIS ? f->gateThr < HUGE_VAL : f->gateThr < 2.0; }
MahaArgs mahaArgs(const eqf_filter* f) {
    return MahaArgs{f->lmc, static_cast<const double*>(f->Sigma[f->pS]), f->sigmaStride, f->ld, f->set.measurementVariance};
}
// The report of filter b: its first n landmarks (ids as the host holds them BEFORE it applies the decision) with the statistics the device left
// in pinned memory; `tripped`: the device acted on them (a filter it did not flag has none above the threshold anyway)
void recordGate(eqf_filter* f, int b, int n, bool tripped) {
    auto& r = f->report[b];
    n = std::min(n, int(f->ids[b].size()));
    const double* st = f->hChord + (size_t)b * f->cap;
    r.ids.assign(f->ids[b].begin(), f->ids[b].begin() + n);
    r.stat.assign(st, st + n);
    r.removed.assign(n, 0);
    if (tripped)
        for (int i = 0; i < n; ++i) r.removed[i] = st[i] > f->gateThr;
}

// Slot of the record ring holding `recs` ([B]) on the device; B == 1 passes the record inline.
int stageRecs(eqf_filter* f, const ImuRec* recs, const ImuRec** dev, int* slotOut) {
    *slotOut = -1;
    if (f->B == 1) {
        *dev = nullptr;
        return EQF_OK;
    }
    const int slot = int(f->ringCount++ % kRing);
    if (f->ringUsed[slot]) HIPC(hipEventSynchronize(f->evRing[slot]));
    std::memcpy(f->hRing + (size_t)slot * f->B, recs, sizeof(ImuRec) * f->B);
    HIPC(hipMemcpyAsync(f->dRing + (size_t)slot * f->B, f->hRing + (size_t)slot * f->B, sizeof(ImuRec) * f->B,
        hipMemcpyHostToDevice, f->stream));
    *dev = f->dRing + (size_t)slot * f->B;
    *slotOut = slot;
    return EQF_OK;
}
int releaseSlot(eqf_filter* f, int slot) {
    if (slot < 0) return EQF_OK;
    HIPC(hipEventRecord(f->evRing[slot], f->stream));
    f->ringUsed[slot] = true;
    return EQF_OK;
}

void mirrorStep(eqf_filter* f, const double* stamps, bool isImu, int* status);

// integrateUpToTime on the device + host mirror of its control flow.  devRecs == nullptr -> inline (B == 1).
int launchPropagate(eqf_filter* f, const ImuRec* devRecs, const ImuRec& inl, const double* stamps, bool isImu, bool doRiccati,
    int* status) {
    f->csValid = false;  // (a single step moves Sigma: columns of C Sigma / S left by an earlier burst are no longer the update's)
    PropArgs a{};
    a.gin = f->g[f->pG];
    a.gout = f->g[f->pG ^ 1];
    a.p0 = f->p0;
    a.Qin = f->Q[f->pG];
    a.Qout = f->Q[f->pG ^ 1];
    a.Sin = f->Sigma[f->pS];
    a.Sout = f->Sigma[f->pS ^ 1];
    a.recs = devRecs;
    a.inl = inl;
    a.errflag = f->errflag;
    a.sigmaStride = f->sigmaStride;
    a.cap = f->cap;
    a.ld = f->ld;
    a.NT = std::max(1, (maxN(f) + kTileLm - 1) / kTileLm);
    a.isImu = isImu ? 1 : 0;
    a.doRiccati = doRiccati ? 1 : 0;
    a.prm = f->prm;
    const dim3 block(256);
    int rc = EQF_OK;
    if (f->densePropagate && doRiccati) {
        // dense backend: F and Bn from the same linearisation blocks, then two MFMA GEMMs; k_propagate below only
        // does the group step and the scalar bookkeeping
        a.sigmaExternal = 1;
        const int nmax = maxN(f), nv = kLm0 + 3 * nmax, nt = (nv + 63) / 64;
        const long long bStride = (long long)f->nTot * 6;
        // (128 x 64 tiles -- twice the MFMAs per staged operand byte -- measured SLOWER than 64 x 64 at N = 1000: fp64 43.6 vs 50.4 TFLOP/s,
        // fp32 73.5 vs 89.4: fewer, fatter workgroups leave a poor last wave; removed in round 5)
        const int ntr = nt;
        rc = profiled(f, EQF_PROF_DENSE, [&] {
            auto go = [&](auto zero) {
                typedef decltype(zero) TT;
                hipLaunchKernelGGL(k_dense_build<TT>, dim3(nmax + 1, f->B), block, 0, f->stream, a, (TT*)f->dF, (TT*)f->dBn, f->sigmaStride, bStride);
                {
                    hipLaunchKernelGGL((k_dense_gemm<TT, false, 64>), dim3(nt, ntr, f->B), block, 0, f->stream, a.gin, a.recs, a.inl,
                        (const TT*)f->dF, (const TT*)a.Sin, (TT*)f->dG, (const TT*)nullptr, f->sigmaStride, bStride, f->ld, f->prm);
                    hipLaunchKernelGGL((k_dense_gemm<TT, true, 64>), dim3(nt, ntr, f->B), block, 0, f->stream, a.gin, a.recs, a.inl,
                        (const TT*)f->dG, (const TT*)f->dF, (TT*)a.Sout, (const TT*)f->dBn, f->sigmaStride, bStride, f->ld, f->prm);
                }
            };
            if (f->precision == EQF_PRECISION_F32) go(0.0f);
            else go(0.0);
        });
        if (rc) return rc;
    }
    a.blk = f->dBlk;
    a.blkCommon = f->dBlkCommon;
    // Split path (builder + lean streaming kernel) when there are enough tiles for occupancy to matter; a single small
    // filter keeps the fused single-launch kernel (one kernel boundary less per step).
    // (measured cross-over on the 256-CU part: 2500 tiles = ten per CU -- 16 filters of N = 200, N >= 800)
    const bool split = f->splitPropagate >= 0 ? f->splitPropagate != 0 : (long long)a.NT * a.NT * f->B >= 10LL * std::max(f->numCUs, 1);
    rc = profiled(f, EQF_PROF_PROPAGATE, [&] {
        if (split) {
            const dim3 bgrid((std::max(1, maxN(f)) + 63) / 64 + 1, f->B);  // landmark workgroups + the scalar-state workgroup
            // builder (blocks + G rows + group step + scalar state), then everything of Sigma by the lean streaming kernel
            const int nmx = std::max(1, maxN(f));
            const dim3 sgrid((nmx + 255) / 256, (nmx + kStreamRows - 1) / kStreamRows, f->B);
            if (f->precision == EQF_PRECISION_F32) {
                hipLaunchKernelGGL(k_build_blocks<float>, bgrid, dim3(128), 0, f->stream, a);
                hipLaunchKernelGGL(k_riccati_stream<float>, sgrid, block, 0, f->stream, a);
            } else {
                hipLaunchKernelGGL(k_build_blocks<double>, bgrid, dim3(128), 0, f->stream, a);
                hipLaunchKernelGGL(k_riccati_stream<double>, sgrid, block, 0, f->stream, a);
            }
        } else {
            // fused kernel: tiles + base-block workgroup + scalar-state workgroup + NT row-tail + NT column-tail workgroups (see k_propagate)
            // + one workgroup per 64 landmarks (group step)
            const dim3 fgrid(a.NT * a.NT + 2 + 2 * a.NT + (std::max(1, maxN(f)) + 63) / 64, f->B);
            if (f->precision == EQF_PRECISION_F32) hipLaunchKernelGGL(k_propagate<float>, fgrid, block, 0, f->stream, a);
            else hipLaunchKernelGGL(k_propagate<double>, fgrid, block, 0, f->stream, a);
        }
    });
    if (rc) return rc;
    HIPC(hipGetLastError());
    f->pG ^= 1;
    f->pS ^= 1;
    if (isImu) std::fill(f->devInit.begin(), f->devInit.end(), 1);
    mirrorStep(f, stamps, isImu, status);
    return EQF_OK;
}

// Until every filter has seen its first IMU sample (lazy initialisation, VIOFilter.cpp:122-124) calls are not queued: the
// generic schedule of the builder then only ever runs single steps, and everything after it is the fast schedule -- so
// the arithmetic of a step never depends on where the bursts are cut.
bool allDevInit(const eqf_filter* f) {
    for (char c : f->devInit)
        if (!c) return false;
    return true;
}

// K steps in two launches (eqf_burst.hpp).  Steps 0 .. K-1 read devRecs[s * recStride + b] (or inl[s], one filter); with
// visionLast the last step is the vision call's integrateUpToTime, its record visRec[b] (or inl[K-1]).
int launchBurst(eqf_filter* f, int K, const ImuRec* devRecs, long long recStride, const ImuRec* inl, bool visionLast, const ImuRec* visRec) {
    if (K <= 0) return EQF_OK;
    BurstArgs a{};
    a.gin = f->g[f->pG];
    a.gout = f->g[f->pG ^ 1];
    a.p0 = f->p0;
    a.Qin = f->Q[f->pG];
    a.Qout = f->Q[f->pG ^ 1];
    a.Sin = f->Sigma[f->pS];
    a.Sout = f->Sigma[f->pS ^ 1];
    a.recs = devRecs;
    a.recStride = recStride;
    a.visRec = visRec;
    if (inl) std::memcpy(a.inl, inl, sizeof(ImuRec) * K);
    a.K = K;
    a.visionLast = visionLast ? 1 : 0;
    a.errflag = f->errflag;
    a.sigmaStride = f->sigmaStride;
    a.cap = f->cap;
    a.ld = f->ld;
    a.colRec = f->dColRec;
    a.rowRec = f->dRowRec;
    a.steps = f->dSteps;
    a.colStep = (int)burstRecStep((long long)kColRec * f->cap);
    a.rowStep = (int)burstRecStep((long long)kBlkRec * f->cap);
    a.prm = f->prm;
    const int nmx = maxN(f);
    // builder: 4 landmarks per workgroup (its eight stages on eight wavefronts, shortest tick) while that launch fits the chip,
    // 16 per workgroup (four panel waves, full lanes) otherwise
    const int cus = std::max(f->numCUs, 1);
    // (the fused launch -- 4-landmark builders + one-row block workgroups -- is deadlock-free on any grid: up to fusedMaxPerCU workgroups per CU)
    int rb1 = 0;
    const bool fusedFits = f->burstFused && nmx > 0 && f->precision != EQF_PRECISION_F32 && f->dBuildFlags &&
                           (double)((nmx + 3) / 4 + ringTiles(nmx, 1, &rb1)) * f->B <= f->fusedMaxPerCU * cus;
    // (round 6: 8 per workgroup -- two panel waves, every serial stage still on a wave of its own -- while THOSE builders have a CU each)
    const int lm = f->burstLm ? f->burstLm
                              : (((long long)((nmx + 3) / 4) * f->B <= cus || fusedFits) ? 4 : ((long long)((nmx + 7) / 8) * f->B <= cus ? 8 : 16));
    const dim3 bgrid(std::max(1, (nmx + lm - 1) / lm), f->B);
    // (round 5: the 4-landmark builder built for two workgroups per CU so that 8 filters keep its short ticks -- 400 workgroups on 512 slots --
    // measured: 70.9 against 71.0 us per burst, nothing; not kept)
    const bool occ2 = lm == 16 && (long long)bgrid.x * bgrid.y > cus;
    // rows per wavefront of the block kernel: one while the launch cannot fill the chip anyway (latency), four once the
    // column constants of a lane are worth sharing between several of its blocks.  (Two rows: 286 VGPRs, one wave per SIMD
    // like four rows but half their reuse -- measured slower than both at every size, N = 200 x 2..64 filters, N = 400..4000.)
    const long long waves1 = (long long)((nmx + 63) / 64) * nmx * f->B;
    // (cross-over measured on the 256-CU part at 2800 wave-blocks = 11 per CU: four filters of N = 200, N >= 400)
    // (in between -- the four-row tiles of the launch would not even give every CU two workgroups: 4 .. 12 filters of N = 200 -- two rows per
    // wavefront, twice the workgroups: 4 filters 62.8 -> 51.4 us per burst, 8: 75.7 -> 71.1, 12: 94.0 -> 89.6; 16: 101 -> 106)
    int rowTiles4 = 0;
    const int R = f->burstRows ? f->burstRows
                               : ((waves1 <= 11LL * cus || fusedFits) ? 1 : ((long long)ringTiles(nmx, 4, &rowTiles4) * f->B <= 3LL * cus / 2 ? 2 : 4));
    const dim3 rgrid(ringTiles(nmx, R, &a.ringBy), f->B);  // (the tiles on and below the diagonal)
    // every filter past its lazy initialisation (VIOFilter.cpp:122-124): the schedule with the precomputed step halves
    const bool fast = allDevInit(f);
    // the latency case in ONE launch: the block workgroups consume a step's records as soon as the builders have them in memory
    // (k_burst_fused).  Only while every workgroup of the launch has a CU of its own; fp64.
    const bool fused = f->burstFused && fast && lm == 4 && R == 1 && nmx > 0 && f->precision != EQF_PRECISION_F32 && f->dBuildFlags &&
                       fusedFits && (int)bgrid.x <= f->nBuildCap - 1088;
    if (fused) {
        if (f->burstEpoch >= (1 << 25)) {  // (flags are epoch * 32 + steps: start over long before the int wraps)
            HIPC(hipMemsetAsync(f->dBuildFlags, 0, sizeof(int) * f->nBuildCap * kFlagReplicas * f->B, f->stream));
            f->burstEpoch = 0;
        }
        a.buildFlags = f->dBuildFlags;
        a.epoch = ++f->burstEpoch;
        a.nBuild = (int)bgrid.x;
        a.nBuildCap = f->nBuildCap;
    }
    f->csValid = false;
    // (measured, round 5, steps/s with / without, profiles/r05_cs_in_burst.txt: 64 filters of N = 200 506.6 k / 497.1 k -- prep launch 117 -> 63 us,
    // block kernel +23 us; N = 1000 7965 / 7887; 16 filters 439.4 / 439.6 k, 8 filters 325.1 / 325.5 k: what the prep launch saves the block
    // kernel's extra stores cost; 2 filters, whose prep work hides inside the update launch, 119.3 / 120.5 k.  So: with the four-row tiles of
    // the throughput sizes; "cs_in_burst" = 2 forces it on every two-launch burst -- the bitwise tests do)
    if (visionLast && !fused && nmx > 0 && (f->csInBurst == 2 || (f->csInBurst && R == 4)) && f->YW && f->SA) {
        a.csOut = 1;
        a.YW = f->YW; a.SA = f->SA; a.lmc = f->lmc;
        a.ldY = f->ldY; a.ldS = f->ldS; a.strideY = f->strideY; a.strideS = f->strideS;
    }
    if (visionLast || f->lastBurstShape[6] == 0) {  // (the bursts that matter to a frame: the ones a vision step closes)
        const int shape[8] = {lm, R, fused ? 1 : 0, a.csOut, (int)bgrid.x, (int)rgrid.x, K, 0};
        std::copy(shape, shape + 8, f->lastBurstShape);
    }
    const int rc = profiled(f, EQF_PROF_BURST, [&] {
        if (fused) {
            hipLaunchKernelGGL((k_burst_fused<double>), dim3(bgrid.x + rgrid.x, f->B), dim3(kBuildThreads), 0, f->stream, a);
            return;
        }
        auto go = [&](auto zero) {
            typedef decltype(zero) TT;
            if (fast && lm == 4) hipLaunchKernelGGL((k_burst_build<TT, true, 4>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else if (fast && lm == 8) hipLaunchKernelGGL((k_burst_build<TT, true, 8>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else if (lm == 8) hipLaunchKernelGGL((k_burst_build<TT, false, 8>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else if (fast && occ2) hipLaunchKernelGGL((k_burst_build<TT, true, 16, true>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else if (fast) hipLaunchKernelGGL((k_burst_build<TT, true, 16>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else if (lm == 4) hipLaunchKernelGGL((k_burst_build<TT, false, 4>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            else hipLaunchKernelGGL((k_burst_build<TT, false, 16>), bgrid, dim3(kBuildThreads), 0, f->stream, a);
            if (nmx > 0) {
                // (the four wavefronts of a workgroup share a step's column constants through an LDS ring)
                if (R == 1) hipLaunchKernelGGL((k_burst_riccati_ring<TT, 1>), rgrid, dim3(256), 0, f->stream, a);
                else if (R == 2 && f->ringAhead2) hipLaunchKernelGGL((k_burst_riccati_ring<TT, 2, true>), rgrid, dim3(256), 0, f->stream, a);
                else if (R == 2) hipLaunchKernelGGL((k_burst_riccati_ring<TT, 2, false>), rgrid, dim3(256), 0, f->stream, a);
                else hipLaunchKernelGGL((k_burst_riccati_ring<TT, 4>), rgrid, dim3(256), 0, f->stream, a);
            }
        };
        if (f->precision == EQF_PRECISION_F32) go(0.0f);
        else go(0.0);
    }, K);
    if (rc) return rc;
    HIPC(hipGetLastError());
    f->pG ^= 1;
    f->pS ^= 1;
    f->csValid = a.csOut != 0;
    if (K - (visionLast ? 1 : 0) > 0) std::fill(f->devInit.begin(), f->devInit.end(), 1);
    return EQF_OK;
}

// (Round 5, measured and dropped: launching the first call queued on an IDLE device at once -- one hipStreamQuery per burst -- so that a run that
// starts from a synchronised handle does not leave the device idle while a frame's calls are queued.  The query costs the host 3 us, a one-step
// burst 15 us of device time: the driver's 20-step shape 369 -> 393 us, steady state 65.0 -> 64.1 k steps/s.  scripts/short_run_trace.py)
bool burstEligible(const eqf_filter* f, bool isImu) {
    return f->burstMax > 0 && !f->densePropagate && (!isImu || !f->set.fastRiccati);
}

// launch the queued IMU steps (optionally closed by the integrateUpToTime of a vision call)
int flushBurstWith(eqf_filter* f, bool visionLast, const ImuRec* visDev, const ImuRec* visInl) {
    auto& q = f->burst;
    const int nImu = q.kind ? q.cnt : 0, K = nImu + (visionLast ? 1 : 0);
    if (K == 0) return EQF_OK;
    HIPC(hipSetDevice(f->device));
    ImuRec inl[kBurstMax];
    const ImuRec* dev = nullptr;
    if (q.kind == 1) dev = f->sImu + (size_t)q.k0 * f->B;
    else if (q.kind == 2) std::memcpy(inl, q.inl, sizeof(ImuRec) * nImu);
    if (visionLast && !visDev) inl[K - 1] = *visInl;
    q.kind = 0;
    q.cnt = 0;
    return launchBurst(f, K, dev, f->B, inl, visionLast, visDev);
}
int flushBurst(eqf_filter* f) { return f->burst.kind ? flushBurstWith(f, false, nullptr, nullptr) : EQF_OK; }

// host mirror (VIOFilter.cpp:120-131, :146-152, :207)
void mirrorStep(eqf_filter* f, const double* stamps, bool isImu, int* status) {
    for (int b = 0; b < f->B; ++b) {
        int st = EQF_OK;
        if (isImu) f->init[b] = 1;  // lazy initialisation happens on the first IMU sample (:122-124)
        if (f->curTime[b] < 0) st = EQF_SKIPPED_BEFORE_FIRST_IMU;
        else if (!(stamps[b] - f->curTime[b] > 0)) st = EQF_SKIPPED_NONPOSITIVE_DT;
        if (st == EQF_OK || isImu) f->curTime[b] = stamps[b];
        if (!isImu && st == EQF_OK && !f->init[b]) st = EQF_SKIPPED_NOT_INITIALISED;
        if (status) status[b] = st;
    }
}

UpdArgs makeUpdArgs(eqf_filter* f, const double* bearings, long long bearStride, const int* perm) {
    UpdArgs a{};
    a.g = f->g[f->pG];
    a.p0 = f->p0;
    a.lmc = f->lmc;
    a.Q = f->Q[f->pG];
    a.Sin = f->Sigma[f->pS];
    a.Sout = f->Sigma[f->pS ^ 1];
    a.sigmaStride = f->sigmaStride;
    a.cap = f->cap;
    a.ld = f->ld;
    a.bearings = bearings;
    a.bearStride = bearStride;
    a.perm = perm;
    a.SA = f->SA; a.SL = f->SL; a.YW = f->YW; a.YO = f->YO;
    a.ldS = f->ldS; a.ldY = f->ldY; a.strideS = f->strideS; a.strideY = f->strideY;
    a.EA = f->EA; a.EL = f->EL; a.ZW = f->ZW; a.ZO = f->ZO;
    a.ldE = f->ldE; a.ldZ = f->ldZ; a.strideE = f->strideE; a.strideZ = f->strideZ;
    a.dbgDelta = f->dbgDelta;
    a.dbgGamma = f->dbgGamma;
    a.dbgGammaTot = f->dbgGammaTot;
    a.red = f->red;
    a.errflag = f->errflag;
    a.resCounters = f->dResCounters;
    a.prm = f->prm;
    a.csInBurst = f->csValid ? 1 : 0;
    return a;
}

// Role table of k_chol_resident for chains of nbS / nbE block columns (wtS right-hand-side column tiles in the S-chain):
// block index = dependency order -- group s holds the workgroups whose last step consumes D[s]; they only wait for groups < s.
// fold: the prep work runs as roles of the same launch (ResArgs::nPrep), so the chains' first diagonal blocks are roles too (F0, in front).
// front (fold on a grid larger than the chip): the first diagonal blocks and the row heads / interior tiles of the E-chain's first `front`
// dependency groups go in FRONT of the prep roles (ResArgs::nFront): they read Sigma only, wait for nothing the prep roles write, and the
// E-chain -- the update's critical path -- starts at t = 0 instead of behind the prep workgroups of all filters.
// border (the co-resident builds with eqf_debug_option "res_border" on): filters that carry the lift's regressors as border rows of the
// E-chain's last block row need no right-hand-side role of that chain except the last one, which runs the lift.  The kernel decides filter
// by filter (a role nobody needs returns at once); the table leaves out what NO filter of the batch needs (border::omitMask) -- only when the
// device will find the host's landmark counts.
int buildRoles(eqf_filter* f, int Nmax, bool fold, int front = 0, bool border = false) {
    const int nbS = roundUp(sDim(Nmax), kSB) / kSB, nbE = roundUp(eDim(Nmax), kSB) / kSB, wtS = roundUp(yCols(Nmax), kSB) / kSB;
    const int key = (fold ? 1 << 30 : 0) | (front << 27) | (nbS << 18) | (nbE << 9) | wtS;  // the table only changes when a chain crosses a 64-block boundary
    unsigned long long omit = 0;
    if (border && f->countsExact) {
        std::vector<int> counts(f->B);
        for (int b = 0; b < f->B; ++b) counts[b] = int(f->ids[b].size());
        omit = border::omitMask(counts.data(), f->B, nbE);
    }
    if (f->rolesN == key && f->rolesOmit == omit) return EQF_OK;
    std::vector<ResRole> r;
    if (fold) {
        r.push_back({1, 6, 0, 0});
        r.push_back({0, 6, 0, 0});
        for (int s = 0; s < std::min(front, nbE - 1); ++s) {
            r.push_back({1, 0, s + 1, 0});
            for (int R = s + 2; R < nbE; ++R) r.push_back({1, 1, R, s});
        }
    }
    f->rolesFront = fold ? int(r.size()) : 0;
    if (!(fold && front > 0)) f->rolesFront = 0;
    for (int s = 0; s < std::max(nbS, nbE); ++s)
        for (int kind = 1; kind >= 0; --kind) {  // the E-chain (the longer one) first
            const int nb = kind ? nbE : nbS, wt = kind ? 1 : wtS;
            if (s >= nb) continue;
            const bool moved = fold && kind == 1 && s < front;  // (its row head and interior tiles are in front; the right-hand-side tile waits for the prep roles)
            if (s + 1 < nb && !moved) r.push_back({kind, 0, s + 1, 0});
            for (int R = s + 2; R < nb && !moved; ++R) r.push_back({kind, 1, R, s});
            for (int t = 0; t < wt; ++t)
                if (!(kind == 1 && ((omit >> s) & 1ull))) r.push_back({kind, 2, t, s});
        }
    // fault injection (eqf_debug_drop_role): the matching role gets an index beyond every chain -- its workgroup returns at once (`R >= nb`)
    // and the flag it owes is never published: the hand-off time-out path of the kernel, on demand
    if (f->dropRole[0] >= 0)
        for (auto& q : r)
            if (q.kind == f->dropRole[0] && q.role == f->dropRole[1] && q.R == f->dropRole[2] && q.C == f->dropRole[3]) q.R = 1 << 20;
    HIPC(hipStreamSynchronize(f->stream));  // (the last update may still read the table)
    const workspace::Want w[] = {want(f->dRoles, sizeof(ResRole) * std::max<size_t>(r.size(), 1), &f->rolesBytes)};
    int rc = reserveSlots(f, w);
    if (rc) return rc;
    HIPC(hipMemcpy(f->dRoles, r.data(), sizeof(ResRole) * r.size(), hipMemcpyHostToDevice));
    f->rolesN = key;
    f->rolesOmit = omit;
    f->rolesCount = int(r.size());
    return EQF_OK;
}

// ---- The launch shape of one update: decided once, from the handle and the largest landmark count of the batch, before anything is
// launched (the prep launch already needs to know whether anybody reads EA's block column 0).  The launches below only read it.
struct UpdateShape {
    int nbS, nbE, wtS, nv;  // 64-wide block columns of the S- and of the E-chain, right-hand-side column tiles of the S-chain; rows of Sigma in use
    // prep work (a launch of its own, or roles of k_chol_resident: `fold`): landmark wavefronts per workgroup, padded row length of their LDS
    // image, landmark workgroups, workgroups of the E-chain's operand, LDS bytes of a landmark workgroup, the launch built for two workgroups per CU
    int wpb, nvPad, lmBlocks, eBlocks;
    size_t prepLds;
    bool occ2Prep;          // (B >= 4 and more workgroups than CUs)
    bool embed;             // downdate + innovation lift ride in the chain launches
    bool splitChain;        // per-column launches: panel launch + update launches that also solve the next block column (else fused launches)
    bool resident;          // one launch for both chains (k_chol_resident); else one launch per block column
    bool residentFits;      // ... and its whole grid is co-resident
    bool fold;              // ... with the prep work as roles of the same launch
    int front;              // ... and this many dependency groups of the E-chain in front of the prep roles (buildRoles)
    bool pipeHeads, occ2;   // builds of k_chol_resident: row heads with the pipelined panel loop, two workgroups per CU
    int eFromSigma;         // UpdArgs::eFromSigma
    bool small;             // downdate: 32 x 32 tiles (4x the workgroups) instead of 64 x 64
    int ddNt, ddTiles;      // ... tiles per edge, tiles
    int i8Slices;           // ... on the integer pipe with this many slices (0: fp64)
    bool tailLaunch, tailLift;  // ... as a launch of its own behind the chains; the innovation lift rides in it
};

int updateShape(eqf_filter* f, int Nmax, UpdateShape& s) {
    const int B = f->B;
    const bool f64 = f->precision != EQF_PRECISION_F32;
    // Factorisation kernels: k_chol_step64 / k_chol_resident (64-wide block columns, register-chained MFMA panel solves).  (The 32-wide
    // family of round 1 -- k_chol_step<INVERSE>, k_update_reduce, a separate prep launch -- was dominated at every size measured and has
    // been removed in round 3; the cross-checks of a factorisation are now the other launch shapes of the same mathematics -- resident
    // vs per-column launches bitwise, fused vs split chain to rounding -- and the fp64 oracle of the tests.)
    s.nbS = roundUp(sDim(Nmax), kSB) / kSB, s.nbE = roundUp(eDim(Nmax), kSB) / kSB, s.wtS = roundUp(yCols(Nmax), kSB) / kSB;
    s.nv = kLm0 + 3 * Nmax;
    const int mp = roundUp(sDim(Nmax), kSB), nep = roundUp(eDim(Nmax), kSB);
    s.nvPad = roundUp(std::min(s.nv, kLm0 + 3 * kPrepLmChunk), 16);
    const size_t perWave = size_t(2) * s.nvPad * sizeof(double);
    s.wpb = int(std::min<size_t>(4, (150 * 1024) / perWave));
    if (s.wpb < 1) return EQF_ERR_CAPACITY;
    s.lmBlocks = (mp / 2 + s.wpb - 1) / s.wpb, s.eBlocks = nep / kNB;
    s.prepLds = perWave * s.wpb;
    s.occ2Prep = B >= 4 && (long long)(s.lmBlocks + s.eBlocks + 2) * B > f->numCUs;
    // The reductions ride along in the rhs workgroups; the downdate and the innovation lift ride along too when every filter's S-chain
    // is shorter than its E-chain (always, except for a handful of landmarks)
    bool eLonger = s.nbS < s.nbE;
    for (int b = 0; b < B && eLonger; ++b) {
        const int Nb = int(f->ids[b].size());
        if (Nb > 0 && roundUp(sDim(Nb), kSB) >= roundUp(eDim(Nb), kSB)) eLonger = false;
    }
    // Per-column launches: fused launches (each tile solves its own panel blocks) while a launch is bound by the serial diagonal chain;
    // panel + update launches (every panel block solved once, 2 workgroups per CU) once it is bound by throughput
    // (measured on the 256-CU part: 1500 workgroups = six per CU -- N = 200 from 8 filters on, N >= ~600)
    const int nblk64 = s.nbS * s.nbS + s.wtS * s.nbS + s.nbE * s.nbE + s.nbE;
    s.splitChain = f->cholSplit >= 0 ? f->cholSplit != 0 : (long long)nblk64 * B >= 6LL * std::max(f->numCUs, 1);
    // ONE launch for the whole factorisation part, k_chol_resident.  While its grid fits the chip every workgroup is resident (one small
    // filter, the latency case).  Beyond co-residency the grid is interleaved (filter index fastest: all filters advance together, group
    // by group), the role table's block order keeps the roles deadlock-free and nothing waits for later workgroups.  Its workgroups mostly
    // wait for hand-offs, so the chip carries several per CU without slowing the chains down; the downdate tiles are workgroups of their
    // own at the end of the grid.  History of the switch-over (round 3, steps/s, per-column launches -> this): first up to 10 roles per CU
    // (2 .. 16 filters of N = 200: 89 -> 107 k, 132 -> 202 k, 226 -> 298 k, 340 -> 373 k), then ONE filter up to ~26 roles per CU, whose
    // per-column launches sit on the latency floor of the diagonal workgroup (N = 600: 11.7 k -> 19.7 k, N = 1000: 5.2 k -> 6.3 k), and
    // finally: since the build for two workgroups per CU (k_chol_resident's OCC2, late in round 3) the resident kernel wins at EVERY size
    // measured -- 24 / 32 / 64 / 96 filters of N = 200: 386 -> 447 k, 410 -> 479 k, 453 -> 509 k, 478 -> 507 k steps/s; one filter of
    // N = 1500 / 2000 / 3000 / 4000: 2.23 -> 2.85 k, 1053 -> 1335, 344 -> 406, 151 -> 174 -- so it runs whenever its buffers exist and
    // the E-chain is the longer one, on a grid of any size; the per-column launches remain for EQF_CHOL_RESIDENT=0 / EQF_CHOL_SPLIT=1 and
    // for filters whose chains are equally long (a handful of landmarks).
    s.resident = eLonger && f->cholResident && f->cholSplit <= 0 && f->dReadyA;
    // the downdate on the integer pipe (eqf_set_option "downdate_slices"): never inside the chain launches -- k_chol_resident runs without its
    // downdate tiles, the per-column shapes without `embed` -- but as the tail launch, for every launch shape
    s.i8Slices = f64 ? f->ddSlices : 0;
    s.embed = eLonger && (s.resident || !s.i8Slices);
    // co-residency of the whole grid by the occupancy calculation (one workgroup per CU with the 119 KB LDS image), not by
    // the CU count alone: the in-kernel downdate waits for workgroups with HIGHER block indices while holding its CU
    if (s.resident && f->residentPerCU < 0) {
        int nblk = 0;
        const void* fn = f64 ? reinterpret_cast<const void*>(&k_chol_resident<double>) : reinterpret_cast<const void*>(&k_chol_resident<float>);
        HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, fn, 256, sizeof(Step64Lds)));
        f->residentPerCU = std::max(nblk, 0);
    }
    auto chainRoles = [](int nb, int wt) { return (nb - 1) + (nb - 1) * (nb - 2) / 2 + wt * nb; };
    const int rolesAll = chainRoles(s.nbS, s.wtS) + chainRoles(s.nbE, 1);
    s.residentFits = s.resident && (long long)rolesAll * B <= (long long)f->residentPerCU * f->numCUs;
    // A co-resident grid (one small filter: the latency case): the prep work -- residuals, C Sigma, S, the lift rows, the chains' first
    // diagonal blocks -- runs as roles of the SAME launch (ResArgs::nPrep, role F0).  The E-chain's diagonal-factor chain, the critical
    // path of the update, needs nothing of it (Sigma_e is Sigma[6:, 6:]: its tiles are read straight from Sigma) and starts at t = 0
    // instead of behind a 12 us launch and a dispatch gap; the S-chain and the right-hand sides wait for the prep roles' flags.
    // (the FOLD build only exists for fp64: the fp32 mode keeps the prep launch)
    const bool foldable = s.resident && f64 && f->cholResident < 2 && s.nbE > 1 && f->dPrepFlags && s.lmBlocks + s.eBlocks <= f->nPrepCap;
    const bool foldFits = foldable && f->resFoldPrep && s.residentFits && s.prepLds <= sizeof(Step64Lds);
    // Round 5: the same on a grid LARGER than the chip (the PIPEH / OCC2 builds with the prep roles in front; filter index fastest, so the
    // prep workgroups of all filters are dispatched first and wait for nobody).  Measured at N = 200 (profiles/r05_fold_batch.txt, steps/s,
    // prep launch -> prep roles): 2 filters 113.7 k -> 118.6 k; 4: 210.2 -> 210.7 k; 8: 316 -> 321 k (the update launch grows by what the
    // prep launch took: 166 -> 195 us -- the prep workgroups fill the chip first and the E-chains start behind them all the same); 16:
    // 436 -> 419 k; 64: 500 -> 465 k.  With the E-chain's first dependency group IN FRONT of the prep roles (buildRoles' `front`;
    // profiles/r05_fold_front.txt): 4 filters 212 -> 219.6 k, 8 and 16 unchanged -- there the path prep -> S-chain ->
    // right-hand sides -> downdate is as long as the E-chain's, and the prep work is on it wherever it runs.  So: while prep roles + chain
    // roles together are at most four per CU (2 .. 4 filters of N = 200) -- round 6, behind the 8-landmark burst builder and this round's
    // other launches (profiles/r06_fold_batch.txt, best of three, prep launch -> prep roles): 5 filters 234.0 -> 246.0 k, 6: 270.6 -> 283.7 k,
    // 8: 340.4 -> 338.5 k, 10: 362.4 -> 357.0 k, 12: 397.5 -> 390.4 k -- so now up to SIX per CU (2 .. 6 filters of N = 200);
    // EQF_RES_FOLD_PREP=3 forces it on every batch (the bitwise test does), = 2 keeps it to co-resident grids.
    const bool foldBatch = foldable && (f->resFoldPrep == 1 || f->resFoldPrep == 3) && !s.residentFits && s.prepLds <= (size_t)kLdsRes2Bytes &&
                           (f->resFoldPrep == 3 || (long long)(s.lmBlocks + s.eBlocks + rolesAll) * B <= 6LL * f->numCUs);
    s.fold = foldFits || foldBatch, s.front = foldBatch ? 1 : 0;
    // the builds of the kernel: row heads with the pipelined panel loop on grids larger than the chip (PIPEH), two workgroups per CU when
    // the grid is many times the chip (OCC2)
    s.pipeHeads = s.resident && !s.residentFits;
    // (roles per CU by buildRoles' table: the chains' roles, and the two first diagonal blocks when the prep work is folded in)
    const double perCU = double(rolesAll + (s.fold ? 2 : 0)) * B / std::max(f->numCUs, 1);
    // (round 4, measured at N = 200: two per CU wins from 5 filters on -- 5 / 6 / 7 filters 217 -> 227 k, 242 -> 255 k, 270 -> 280 k steps/s -- and
    // loses below: 4 filters 210 -> 195 k; one filter of N = 400, three roles per CU, 33.5 -> 32.5 k)
    s.occ2 = s.pipeHeads && (perCU > 6.0 || (B >= 5 && perCU > 2.4));
    // 2: k_chol_resident reads the E-chain's tiles straight from Sigma, no copy in the prep work -- the FOLD builds, and the OCC2 build from
    // eSigmaMinPerCU roles per CU on; 1: the split chain reads block column 0 of the E-chain there (fp64 only, both)
    const bool eSigma = s.occ2 && perCU > f->eSigmaMinPerCU && f64;
    s.eFromSigma = (s.fold || eSigma) ? 2 : ((!s.resident && s.splitChain && f64) ? 1 : 0);
    // downdate tiling: 64x64 tiles when they fill the chip, 32x32 tiles (4x the workgroups) for a single small filter.  Inside
    // k_chol_resident: 64 x 64 -- a tile costs the same 14 dependent chunk fetches whatever its size, and there are enough finished
    // workgroups to take one each -- except in the FOLD build without PIPEH (co-resident grids: 32 x 32 tiles, see the kernel)
    const int nt64 = (s.nv + 63) / 64, nt32 = (s.nv + 31) / 32;
    s.small = (long long)nt64 * (nt64 + 1) / 2 * B < 2LL * std::max(f->numCUs, 1);
    s.ddNt = (s.resident ? s.fold && !s.pipeHeads : s.small) ? nt32 : nt64;
    s.ddTiles = s.ddNt * (s.ddNt + 1) / 2;
    s.tailLaunch = !s.embed || s.i8Slices;
    s.tailLift = !s.resident;  // (k_chol_resident's roles run the lift whenever that kernel runs)
    return EQF_OK;
}

// Dynamic LDS beyond 64 KB has to be allowed function by function (and device by device: remembered per handle, not per process).  The
// table lists exactly the instantiations that the launches below it name.
int allowUpdateLds(eqf_filter* f) {
    if (f->ldsAttrSet) return EQF_OK;
#ifdef EQF_F64_STAMPS
    const int prepLds = 158 * 1024;  // (the instrumented build keeps factor64's stamps in 1 KB of static LDS)
#else
    const int prepLds = 160 * 1024;
#endif
    const int fullLds = int(sizeof(Step64Lds));
    auto fn = [](auto* kernel) { return reinterpret_cast<const void*>(kernel); };
    const struct { const void* fn; int bytes; } table[] = {
        {fn(&k_update_prep64<float, false>), prepLds},
        {fn(&k_update_prep64<double, false>), prepLds},
        {fn(&k_update_prep64<float, true>), prepLds},
        {fn(&k_update_prep64<double, true>), prepLds},
        {fn(&k_chol_resident<float, false>), fullLds},
        {fn(&k_chol_resident<double, false>), fullLds},
        {fn(&k_chol_resident<float, true>), fullLds},
        {fn(&k_chol_resident<double, true>), fullLds},
        {fn(&k_chol_resident<float, true, true>), kLdsRes2Bytes},
        {fn(&k_chol_resident<double, true, true>), kLdsRes2Bytes},
        {fn(&k_chol_resident<double, false, false, true>), fullLds},
        {fn(&k_chol_resident<double, true, false, true>), fullLds},
        {fn(&k_chol_resident<double, true, true, true>), kLdsRes2Bytes},
        {fn(&k_chol_resident<float, true, false, false, true>), fullLds},
        {fn(&k_chol_resident<double, true, false, false, true>), fullLds},
        {fn(&k_chol_resident<float, true, true, false, true>), kLdsRes2Bytes},
        {fn(&k_chol_resident<double, true, true, false, true>), kLdsRes2Bytes},
        {fn(&k_chol_step64<float, 0>), fullLds},
        {fn(&k_chol_step64<double, 0>), fullLds},
        {fn(&k_chol_step64<float, 1>), fullLds},
        {fn(&k_chol_step64<double, 1>), fullLds},
        {fn(&k_chol_step64<float, 3>), kLdsTailBytes},
        {fn(&k_chol_step64<double, 3>), kLdsTailBytes},
    };
    for (const auto& e : table) HIPC(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes));
    f->ldsAttrSet = true;
    return EQF_OK;
}

// Border rows (ResArgs::border): the co-resident builds of fp64 handles whose downdate runs inside the launch.  Not the fp32 mode and not
// the downdate on the integer pipe: there existing checks hold one filter alone against the per-column launches (bit for bit) and against
// a filter of a batch on a grid larger than the chip (1e-12 on Sigma behind the int8 split, which amplifies last-bit differences of the
// state) -- shapes without the border.
bool useBorder(const eqf_filter* f, const UpdateShape& s) {
    return f->resBorder && s.resident && !s.pipeHeads && f->precision != EQF_PRECISION_F32 && !s.i8Slices;
}

// ONE launch for both chains: the roles of the table buildRoles left, the prep roles in front of them with `fold`, the downdate tiles
// behind them unless the downdate runs on the integer pipe
template <typename T>
int launchChainsResident(eqf_filter* f, const UpdateShape& s, const ChainArgs& cS, const ChainArgs& cE, const UpdArgs& a) {
    ResArgs ra{};
    ra.c0 = cS; ra.c1 = cE; ra.a = a;
    ra.roles = f->dRoles;
    ra.readyA = f->dReadyA; ra.readyY = f->dReadyY; ra.counters = f->dResCounters;
    ra.gammaPart = f->dGammaPart; ra.g11Part = f->dG11Part;
    ra.nbCap = f->nbCap; ra.wtCap = f->wtCap;
    ra.stageFlags = f->dStageFlags;  // (row heads consume D[R-1] stage by stage)
    ra.eFromSigma = s.eFromSigma == 2 ? 1 : 0;
    ra.border = useBorder(f, s) ? 1 : 0;  // (k_chol_resident decides filter by filter)
    if (s.fold) {
        ra.waitD0 = 3;
        ra.nPrep = s.lmBlocks + s.eBlocks;
        ra.nFront = f->rolesFront;
        ra.lmBlocks = s.lmBlocks;
        ra.prepWpb = s.wpb;
        ra.prepNvPad = s.nvPad;
        ra.prepFlags = f->dPrepFlags;
        ra.nPrepCap = f->nPrepCap;
    }
    ra.ddNt = s.ddNt;
    // (the downdate tiles are workgroups of their own behind the roles, also when the whole grid is co-resident: nothing in the kernel
    // waits for a higher block index; a grid larger than what is co-resident must not wait for later workgroups while holding CUs)
    ra.nDdTiles = s.i8Slices ? 0 : s.ddTiles;
    ra.nRoles = f->rolesCount;
    ra.errflag = f->errflag;
    const int perFilter = ra.nPrep + f->rolesCount + ra.nDdTiles;
    ra.rolesPerRow = std::min(perFilter, 32768);
    const dim3 rg(f->B * ra.rolesPerRow, (perFilter + ra.rolesPerRow - 1) / ra.rolesPerRow);
    // Arrival tickets (ResArgs::ticket, the TICKET build): eqf_debug_option "res_tickets" 0 (default) = never, 2 = on every grid larger
    // than the chip that has its prep launch in front (not the FOLD build of 2 - 4 filters), 1 = where they cost least -- grids of at
    // least six times the resident slots (16+ filters of N = 200, N >= ~700), whose workgroups are dispatched long before they are needed;
    // on lightly oversubscribed grids a role is dispatched just in time and the ticket's round trip (~2 us) lands on the critical
    // path at every dependency hop: +12.8 / +7.4 / +14.6 / +3.2 / +8.6 us per update at 2 / 4 / 6 / 8 / 12 filters, +1.1 % at 64, +0.7 %
    // at N = 1000 in one binary (profiles/r06_tickets_ab.txt), 2.3 % against round 5's library on the same box.  OFF by default: the
    // block index with the time-outs as its guard, as in rounds 3 - 5 -- the guarantee is there for whoever wants to pay for it.
    const long long slots = (long long)std::max(f->numCUs, 1) * (s.occ2 ? 2 : 1);
    const bool tickets = f->resTickets == 2 || (f->resTickets == 1 && (long long)rg.x * rg.y >= 6 * slots);
    const bool ticketBuild = s.pipeHeads && !s.fold && tickets && f->dTicket;
    return profiled(f, EQF_PROF_CHOL_RESIDENT, [&] {
        if (ticketBuild) {  // (every workgroup of the launch draws exactly one ticket, padding workgroups included)
            ra.ticket = f->dTicket;
            ra.ticketBase = f->ticketBase;
            f->ticketBase += ra.rolesPerRow * rg.y;  // (per filter)
        }
        const dim3 wg(256);
        const size_t fullLds = sizeof(Step64Lds);
        if (s.fold) {
            if constexpr (std::is_same<T, double>::value) {  // (the FOLD build only exists for fp64: updateShape)
                if (s.occ2) hipLaunchKernelGGL((k_chol_resident<double, true, true, true>), rg, wg, kLdsRes2Bytes, f->stream, ra);
                else if (s.pipeHeads) hipLaunchKernelGGL((k_chol_resident<double, true, false, true>), rg, wg, fullLds, f->stream, ra);
                else hipLaunchKernelGGL((k_chol_resident<double, false, false, true>), rg, wg, fullLds, f->stream, ra);
            }
        } else if (ticketBuild && s.occ2) hipLaunchKernelGGL((k_chol_resident<T, true, true, false, true>), rg, wg, kLdsRes2Bytes, f->stream, ra);
        else if (ticketBuild) hipLaunchKernelGGL((k_chol_resident<T, true, false, false, true>), rg, wg, fullLds, f->stream, ra);
        else if (s.occ2) hipLaunchKernelGGL((k_chol_resident<T, true, true>), rg, wg, kLdsRes2Bytes, f->stream, ra);
        else if (s.pipeHeads) hipLaunchKernelGGL((k_chol_resident<T, true>), rg, wg, fullLds, f->stream, ra);
        else hipLaunchKernelGGL((k_chol_resident<T, false>), rg, wg, fullLds, f->stream, ra);
    });
}

// One launch per block column, split chain: the panel launch of column 0, then update launches that also solve column k+1
// (k_chol_step64<T, 3>); the S-chain's right-hand sides are complete after launch nbS - 2, the downdate joins launch nbS - 1 (`embed`:
// nbS < nbE, so there is one)
template <typename T>
int launchChainsSplit(eqf_filter* f, const UpdateShape& s, const ChainArgs& cS, const ChainArgs& cE, const UpdArgs& a) {
    const int B = f->B;
    int rc = profiled(f, EQF_PROF_CHOL_STEP, [&] {
        const int grid = chainBlocks64(s.nbS, s.wtS, 0, 1) + chainBlocks64(s.nbE, 1, 0, 1);
        hipLaunchKernelGGL((k_chol_step64<T, 1>), dim3(grid, B), dim3(256), sizeof(Step64Lds), f->stream, cS, cE, a, 0, 0, 0, s.embed ? 1 : 0,
            f->errflag);
    }, 1000);
    if (rc) return rc;
    // (A downdate with 128 x 128 tiles -- half the Y traffic per flop -- as a launch of its own was tried here and measured
    // SLOWER: 788 vs 516 us for 64 filters, 48 vs 29.5 ms at N = 4000; 352 registers leave one wave per SIMD.  The 64-wide
    // tiles are not bandwidth-bound: they run at half the fp64 MFMA peak in executed flops.)
    for (int k = 0; k + 1 < std::max(s.nbS, s.nbE); ++k) {
        const int dd = (s.embed && k == s.nbS - 1) ? s.ddTiles : 0;
        // workgroups per filter: 2 diagonal + the tails of block column k+1 + nStream streams over the pure updates
        // (about two per CU over the whole launch; four for ONE large filter: N = 4000 150 -> 154 steps/s) + the downdate tiles; see step3Counts
        int tS, uS, tE, uE;
        step3Counts(s.nbS, s.wtS, k, &tS, &uS);
        step3Counts(s.nbE, 1, k, &tE, &uE);
        const int nStream = std::min(uS + uE, std::max(1, ((B == 1 ? 4 : 2) * f->numCUs + B - 1) / B));
        rc = profiled(f, dd ? EQF_PROF_CHOL_DD : EQF_PROF_CHOL_STEP, [&] {
            // (the last argument, tailsLast = 1: the streams are dispatched before the tails, which only wait)
            hipLaunchKernelGGL((k_chol_step64<T, 3>), dim3(2 + tS + tE + nStream + dd, B), dim3(256), kLdsTailBytes, f->stream, cS, cE, a, k,
                dd ? s.ddNt : 0, s.small ? 1 : 0, s.embed ? 1 : 0, f->errflag, nStream, 1);
        }, k);
        if (rc) return rc;
    }
    return EQF_OK;
}

// One launch per block column, fused: every tile workgroup solves the two panel blocks it needs itself; the downdate joins launch nbS
template <typename T>
int launchChainsFused(eqf_filter* f, const UpdateShape& s, const ChainArgs& cS, const ChainArgs& cE, const UpdArgs& a) {
    for (int k = 0; k < std::max(s.nbS, s.nbE); ++k) {
        const int dd = (s.embed && k == s.nbS) ? s.ddTiles : 0;
        const int rc = profiled(f, dd ? EQF_PROF_CHOL_DD : EQF_PROF_CHOL_STEP, [&] {
            const int grid = chainBlocks64(s.nbS, s.wtS, k, 0) + chainBlocks64(s.nbE, 1, k, 0);
            hipLaunchKernelGGL((k_chol_step64<T, 0>), dim3(grid + dd, f->B), dim3(256), sizeof(Step64Lds), f->stream, cS, cE, a, k, dd ? s.ddNt : 0,
                s.small ? 1 : 0, s.embed ? 1 : 0, f->errflag);
        }, k);
        if (rc) return rc;
    }
    return EQF_OK;
}

template <typename T>
int launchUpdateT(eqf_filter* f, const double* bearings, long long bearStride, const int* perm, int Nmax) {
    UpdArgs a = makeUpdArgs(f, bearings, bearStride, perm);
    f->csValid = false;  // (consumed)
    const int B = f->B;
    UpdateShape s{};
    int rc = allowUpdateLds(f);
    if (!rc) rc = updateShape(f, Nmax, s);
    if (!rc && s.resident) rc = buildRoles(f, Nmax, s.fold, s.front, useBorder(f, s));
    if (rc) return rc;
    a.pad = kSB; a.eFromSigma = s.eFromSigma;
    ChainArgs cS{}, cE{};
    cS.g = a.g; cS.A = f->SA; cS.D = f->SL; cS.W = f->YW; cS.WO = f->YO;
    cS.ldA = f->ldS; cS.ldW = f->ldY; cS.strideA = f->strideS; cS.strideD = f->strideDS; cS.strideW = f->strideY;
    cS.kind = 0; cS.nbMax = s.nbS; cS.wtMax = s.wtS;
    cE.g = a.g; cE.A = f->EA; cE.D = f->EL; cE.W = f->ZW; cE.WO = f->ZO;
    cE.ldA = f->ldE; cE.ldW = f->ldZ; cE.strideA = f->strideE; cE.strideD = f->strideDE; cE.strideW = f->strideZ;
    cE.kind = 1; cE.nbMax = s.nbE; cE.wtMax = 1;
    f->updateEpoch = f->updateEpoch == 0x7fffffff ? 1 : f->updateEpoch + 1;
    cS.flags = f->dFlags; cS.strideF = 2 * f->flagStride; cS.epoch = f->updateEpoch;
    cE.flags = f->dFlags + f->flagStride; cE.strideF = 2 * f->flagStride; cE.epoch = f->updateEpoch;
    // (round 5, measured and dropped: with the burst's operands in place, the landmark work as one LANE per landmark -- 128 per workgroup, the
    // stores from an LDS image -- instead of one wavefront: bit for bit the same and no faster.  Such a workgroup takes 21-31 us (33
    // uncoalesced loads per lane, then the stores) against 12.7 us for the 4-landmark ones, and a launch of 64 filters is three dispatch
    // rounds each as long as its longest workgroup: 63 -> 65 us; N = 1000 18 -> 82 us (one workgroup wrote all the padding rows).
    // profiles/r05_prep_stamps.txt)
    if (!s.fold) rc = profiled(f, EQF_PROF_UPDATE_PREP, [&] {
        // the landmark waves + E-chain operand + two more workgroups per filter that factor the first diagonal block of each chain
        // straight from Sigma (one launch: measured never slower than a separate factor launch, 4..64 filters)
        const dim3 grid(s.lmBlocks + s.eBlocks + 2, B);
        const size_t lds = std::max(s.prepLds, (size_t)kLdsFactorBytes);
        if (s.occ2Prep) hipLaunchKernelGGL((k_update_prep64<T, true>), grid, dim3(256), lds, f->stream, a, cS, cE, s.lmBlocks, s.eBlocks, s.wpb, s.nvPad);
        else hipLaunchKernelGGL((k_update_prep64<T, false>), grid, dim3(256), lds, f->stream, a, cS, cE, s.lmBlocks, s.eBlocks, s.wpb, s.nvPad);
    });
    if (rc) return rc;
    rc = s.resident ? launchChainsResident<T>(f, s, cS, cE, a) : s.splitChain ? launchChainsSplit<T>(f, s, cS, cE, a) : launchChainsFused<T>(f, s, cS, cE, a);
    if (rc) return rc;
    if (s.tailLaunch && s.i8Slices) {
        // split + symmetric product on the integer pipe; the innovation lift rides along in the split launch (`tailLift`)
        I8DdArgs ia{};
        ia.Y = a.YO; ia.ldY = a.ldY; ia.strideY = a.strideY;
        ia.Sin = static_cast<const double*>(a.Sin); ia.Sout = static_cast<double*>(a.Sout); ia.ld = a.ld; ia.sigmaStride = a.sigmaStride;
        ia.g = a.g; ia.dims = nullptr; ia.pad = a.pad; ia.skipCol = 11;
        ia.ws = f->dI8Ws; ia.wsStride = f->i8WsStride; ia.expo = f->dI8Expo; ia.expoStride = i8ddExpoWords(kLm0 + 3 * f->cap);
        ia.B = B; ia.nt = (s.nv + 63) / 64;
        rc = profiled(f, EQF_PROF_DOWNDATE, [&] { launchI8Dd(s.i8Slices, ia, s.tailLift ? &a : nullptr, (s.nv + 31) / 32, f->stream); });
    } else if (s.tailLaunch) {
        // the last workgroup of the launch runs the (independent) innovation-lift / group-update part
        rc = profiled(f, EQF_PROF_DOWNDATE, [&] {
            if (s.small) hipLaunchKernelGGL((k_downdate<T, 32>), dim3(s.ddTiles + 1, B), dim3(256), (downdateLdsBytes<T, 32>()), f->stream, a, s.ddNt, 1);
            else hipLaunchKernelGGL((k_downdate<T, 64>), dim3(s.ddTiles + 1, B), dim3(256), (downdateLdsBytes<T, 64>()), f->stream, a, s.ddNt, 1);
        });
    }
    if (rc) return rc;
    if (f->innovStats && std::is_same<T, double>::value) {
        // (a tail launch of its own, only with the option on: the update's other launches are what they are without it)
        InnovArgs na{};
        na.g = a.g; na.YO = f->YO; na.ldY = f->ldY; na.strideY = f->strideY; na.SL = f->SL; na.strideDS = f->strideDS;
        na.delta = f->dbgDelta; na.lmc = f->lmc; na.Sin = static_cast<const double*>(a.Sin); na.ld = f->ld; na.cap = f->cap;
        na.sigmaStride = f->sigmaStride; na.measurementVariance = f->prm.measurementVariance; na.out = f->dInnov;
        hipLaunchKernelGGL(k_innov_stats, dim3(B), dim3(256), 0, f->stream, na);
    }
    HIPC(hipGetLastError());
    f->pS ^= 1;
    return EQF_OK;
}

int launchUpdate(eqf_filter* f, const double* bearings, long long bearStride, const int* perm, int Nmax) {
    return f->precision == EQF_PRECISION_F32 ? launchUpdateT<float>(f, bearings, bearStride, perm, Nmax)
                                             : launchUpdateT<double>(f, bearings, bearStride, perm, Nmax);
}

// launch(T{}) with T = the handle's Sigma type, for a kernel whose two instantiations take the same arguments (the style of i8WithSlices)
template <typename F>
void withSigmaType(const eqf_filter* f, F&& launch) {
    if (f->precision == EQF_PRECISION_F32) launch(float{});
    else launch(double{});
}

// Batch-wide compaction with host keep-lists keep[b] = old indices that survive (ascending); once the launch is in the stream the host's
// id lists follow.
int compactIds(eqf_filter* f, const frame::Lists& keep) {
    const int B = f->B, cap = f->cap;
    f->csValid = false;
    int* h = nullptr;
    int slot = 0;
    int rcs = stageAcquire(f->stMap, &h, &slot);
    if (rcs) return rcs;
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        h[(size_t)B * cap + b] = int(keep[b].size());
        nmax = std::max(nmax, int(keep[b].size()));
        std::copy(keep[b].begin(), keep[b].end(), h + (size_t)b * cap);
    }
    HIPC(hipMemcpyAsync(f->dMap, h, sizeof(int) * ((size_t)B * cap + B), hipMemcpyHostToDevice, f->stream));  // (map + new counts: one copy)
    HIPC(hipEventRecord(f->stMap.ev[slot], f->stream));
    const int nvn = kLm0 + 3 * nmax;
    int rc = profiled(f, EQF_PROF_CHURN, [&] {
        withSigmaType(f, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_compact<T>, dim3((nvn + 255) / 256, nvn, B), dim3(256), 0, f->stream, f->g[f->pG], f->dMap, f->dNewN, cap,
                static_cast<const T*>(f->Sigma[f->pS]), static_cast<T*>(f->Sigma[f->pS ^ 1]), f->sigmaStride, f->ld, f->p0, f->Q[f->pG], f->lmc,
                f->dScratch);
        });
    });
    if (rc) return rc;
    HIPC(hipGetLastError());
    f->pS ^= 1;
    frame::applyKeep(f->ids, keep);
    return EQF_OK;
}

// perm[b][i] = index into the measurement of state landmark i (or -1)
int uploadPerm(eqf_filter* f, const frame::Lists& perm) {
    const int B = f->B, cap = f->cap;
    // A landmark that was removed as an outlier and comes back is appended at the END of the state: from then on the state's order differs
    // from the measurement's on every frame, with the SAME permutation as long as the set does not change.  Each copy is a blit launch on
    // the stream (4 us + its boundaries; the gate and the update both ask for the permutation: 2.4 copies per frame in the churn leg).
    if (perm == f->permOnDevice) return EQF_OK;
    int* h = nullptr;
    int slot = 0;
    int rc = stageAcquire(f->stPerm, &h, &slot);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        std::fill(h + (size_t)b * cap, h + (size_t)(b + 1) * cap, -1);
        std::copy(perm[b].begin(), perm[b].end(), h + (size_t)b * cap);
    }
    f->permOnDevice.clear();  // (not valid if the copy cannot be enqueued)
    HIPC(hipMemcpyAsync(f->dPerm, h, sizeof(int) * B * cap, hipMemcpyHostToDevice, f->stream));
    HIPC(hipEventRecord(f->stPerm.ev[slot], f->stream));
    f->permOnDevice = perm;
    return EQF_OK;
}

// chord errors (when bearings are given) and squared depths of every landmark of the current estimate -> dChord, dDepth2;
// readback = true also copies them to the host and waits (only the outlier gate needs that: the host owns the ids)
int probe(eqf_filter* f, const double* bearings, long long bearStride, bool withPerm, bool readback, bool speculative = false) {
    const int B = f->B, cap = f->cap;
    const int nmax = std::max(1, maxN(f));
    // with readback the kernel writes the chords straight into pinned host memory (no copy command behind it)
    double* chordDst = (readback || speculative) ? f->hChord.dev : f->dChord;  // (speculative: resolveGate reads them if the gate tripped)
    // (the Mahalanobis statistic only where a gate looks at it: the depth-only probe of addNewAndUpdate stays k_probe)
    const bool maha = f->gateKind == EQF_GATE_MAHALANOBIS && bearings && (readback || speculative);
    int rc = profiled(f, EQF_PROF_CHURN, [&] {
        if (maha)
            hipLaunchKernelGGL(k_probe_maha, dim3((nmax + 127) / 128, B), dim3(128), 0, f->stream, f->g[f->pG], f->p0, f->Q[f->pG], cap, bearings,
                bearStride, withPerm ? f->dPerm : nullptr, chordDst, f->dDepth2, f->gateThr, speculative ? f->hGate.dev : nullptr, mahaArgs(f));
        else
            hipLaunchKernelGGL(k_probe, dim3((nmax + 127) / 128, B), dim3(128), 0, f->stream, f->g[f->pG], f->p0, f->Q[f->pG], cap, bearings,
                bearStride, withPerm ? f->dPerm : nullptr, chordDst, f->dDepth2, f->gateThr, speculative ? f->hGate.dev : nullptr);
    });
    if (rc) return rc;
    if (readback) HIPC(hipStreamSynchronize(f->stream));
    return EQF_OK;
}

// (per-call API: the bearings are still in pinned host memory -- whoever enqueues the first consumer enqueues their copy, with `extra` more
// bytes behind them: k_edit's image)
int flushMeas(eqf_filter* f, size_t extra = 0) {
    if (!f->measPending) return EQF_OK;
    f->measPending = false;
    HIPC(hipMemcpyAsync(f->dMeas, f->hMeas, sizeof(double) * frameImage(f).bearingDoubles() + extra, hipMemcpyHostToDevice, f->stream));
    HIPC(hipEventRecord(f->evMeas, f->stream));
    return EQF_OK;
}

// before a launch that raises hGate: a redo's k_set_update_ok may still have to read the flags of the frame before
int awaitMaskAndClearFlags(eqf_filter* f) {
    if (f->maskPending) {
        HIPC(hipEventSynchronize(f->evMask));
        f->maskPending = false;
    }
    std::fill(f->hGate.get(), f->hGate + f->B, 0);
    return EQF_OK;
}

// ... and behind it: the frame whose gate answer resolveGate() will look at (the route's own fields are the caller's to fill in)
int armGate(eqf_filter* f, bool onDevice, const frame::Meas& m, const double* bearings, long long bearStride) {
    HIPC(hipEventRecord(f->evGate, f->stream));
    f->gate.pending = true;
    f->gate.onDevice = onDevice;
    f->gate.active = m.active;
    f->gate.bearings = bearings;
    f->gate.bearStride = bearStride;
    return EQF_OK;
}

// resolveGate's redo: the update of the filters hGate marks runs after all
int launchSetUpdateOk(eqf_filter* f) {
    hipLaunchKernelGGL(k_set_update_ok, dim3((f->B + 63) / 64), dim3(64), 0, f->stream, f->g[f->pG], f->hGate.dev, f->B);
    HIPC(hipEventRecord(f->evMask, f->stream));
    f->maskPending = true;
    return EQF_OK;
}

// (k_median_depth reads N from the device state, which still holds the old counts: nmx = the largest of them)
int launchMedianDepth(eqf_filter* f, int nmx) {
    return profiled(f, EQF_PROF_CHURN, [&] {
        hipLaunchKernelGGL(k_median_depth, dim3((nmx + 255) / 256, f->B), dim3(256), 0, f->stream, f->g[f->pG], f->dDepth2, f->cap, f->dDepthSel);
    });
}

// nNew landmarks behind the nOld of filter b; the bearing of the j-th is entry permDev[nOld + j] of the filter's measurement (null: nOld + j)
int launchAppend(eqf_filter* f, int b, int nOld, int nNew, const double* depthSel, const double* bearings, const int* permDev) {
    f->csValid = false;
    const long long work = (long long)3 * nNew * (kLm0 + 3 * (nOld + nNew)) * 2;
    const int blocks = int(std::min<long long>(1024, (work + 255) / 256));
    int rc = profiled(f, EQF_PROF_CHURN, [&] {
        withSigmaType(f, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_append<T>, dim3(std::max(1, blocks)), dim3(256), 0, f->stream, f->g[f->pG], b, nOld, nNew, depthSel, (const double*)nullptr,
                f->set.initialSceneDepth, f->set.initialPointVariance, f->cap, bearings, permDev, f->p0,
                f->Q[f->pG], f->lmc, f->errflag, static_cast<T*>(f->Sigma[f->pS]), f->sigmaStride, f->ld);
        });
    });
    if (rc) return rc;
    HIPC(hipGetLastError());
    return EQF_OK;
}

// The whole landmark bookkeeping of the frame in one launch (k_edit, eqf_churn.hpp; round 5) -- the host's keep list, the outlier gate
// evaluated AND acted upon on the device, the new landmarks -- with one upload, and no frame is ever redone.
int visionOneLaunch(eqf_filter* f, const frame::Meas& m, const double* bearings, long long bearStride, int* status, const frame::Lists& keep,
    bool anyLost, bool gateArmed) {
    const int B = f->B, cap = f->cap;
    // (per-call API: the image rides behind the bearings, one copy for both; stream API: a staging ring of its own)
    const bool withMeas = f->measPending;
    const frame::ImageLayout fi = frameImage(f);
    int* h = withMeas ? reinterpret_cast<int*>(f->hMeas + fi.offEdit()) : nullptr;
    int slot = 0;
    int rc = withMeas ? EQF_OK : stageAcquire(f->stEdit, &h, &slot);
    if (rc) return rc;
    // (the new id lists and the "no bearings left" verdicts are committed to the handle only once k_edit is in the stream: an error on
    // the way there -- capacity, a failed copy, a failed launch -- leaves the host's lists describing what the device still holds)
    frame::EditPlan plan;
    if (!frame::editImage(f->ids, keep, m, gateArmed, cap, h, plan)) return EQF_ERR_CAPACITY;  // (cannot happen: every entry point checks nb <= capacity)
    // (a fixed set behind an armed gate: the same image every frame, nothing to upload)
    const size_t nInts = fi.editInts();
    const int* devImage = f->dEdit;
    if (withMeas) {
        rc = flushMeas(f, sizeof(int) * nInts);
        if (rc) return rc;
        devImage = reinterpret_cast<const int*>(f->dMeas + fi.offEdit());
    } else if (f->editOnDevice.size() != nInts || !std::equal(h, h + nInts, f->editOnDevice.begin())) {
        f->editOnDevice.clear();
        HIPC(hipMemcpyAsync(f->dEdit, h, sizeof(int) * nInts, hipMemcpyHostToDevice, f->stream));
        HIPC(hipEventRecord(f->stEdit.ev[slot], f->stream));
        f->editOnDevice.assign(h, h + nInts);
    }
    if (gateArmed) rc = awaitMaskAndClearFlags(f);
    if (rc) return rc;
    EditArgs ea{};
    ea.g = f->g[f->pG];
    ea.in = devImage;
    ea.permOut = f->dPerm;
    ea.B = B; ea.cap = cap;
    ea.bearings = bearings; ea.bearStride = bearStride;
    ea.gateThr = f->gateThr;
    ea.measVar = f->set.measurementVariance;
    ea.gateFlag = gateArmed ? f->hGate.dev : nullptr;
    ea.chordOut = gateArmed ? f->hChord.dev : nullptr;
    ea.depthDefault = f->set.initialSceneDepth; ea.pointVar = f->set.initialPointVariance;
    ea.p0 = f->p0; ea.Q = f->Q[f->pG]; ea.lmc = f->lmc;
    ea.errflag = f->errflag;
    ea.Scur = f->Sigma[f->pS]; ea.Soth = f->Sigma[f->pS ^ 1];
    ea.sigmaStride = f->sigmaStride; ea.ld = f->ld;
    ea.hostFlip = anyLost ? 1 : 0;
    ea.bar = f->dEditBar;
    // (co-resident when an outliers-only compaction may have to wait for its workgroups; a frame whose Sigma the host knows to move
    // anyway waits for nobody: a workgroup per four rows)
    const int coRes = std::max(1, std::min(64, std::max(f->numCUs, 1) / B));
    const int G = (anyLost || !gateArmed) ? std::max(coRes, std::min(1024, (kLm0 + 3 * plan.Nmax + 3) / 4)) : coRes;  // (no gate: nothing can trip)
    rc = profiled(f, EQF_PROF_CHURN, [&] {
        if (gateArmed && f->gateKind == EQF_GATE_MAHALANOBIS)  // (fp64 handles only: eqf_set_outlier_gate)
            hipLaunchKernelGGL((k_edit<double, 1>), dim3(G, B), dim3(256), 0, f->stream, ea);
        else
            withSigmaType(f, [&](auto t) { hipLaunchKernelGGL((k_edit<decltype(t), 0>), dim3(G, B), dim3(256), 0, f->stream, ea); });
    });
    if (rc) return rc;
    HIPC(hipGetLastError());
    f->ids = std::move(plan.newIds);
    if (status)
        for (int b : plan.skipped) status[b] = EQF_SKIPPED_NO_BEARINGS;
    if (anyLost) f->pS ^= 1;
    f->csValid = false;
    f->permOnDevice.clear();  // (dPerm now holds what k_edit made of the upload)
    if (gateArmed) {
        rc = armGate(f, true, m, bearings, bearStride);
        if (rc) return rc;
        f->gate.nKept = plan.nKept;
    }
    if (!plan.anyWork) return EQF_OK;
    f->countsExact = !gateArmed;  // (an armed gate takes its outliers out on the device: the update may find fewer landmarks than the host counts)
    rc = launchUpdate(f, bearings, bearStride, f->dPerm, plan.Nmax);
    f->countsExact = true;
    return rc;
}

// Speculative gate: the probe decides on the device, the frame's new landmarks and the update are enqueued without waiting for the
// answer, and a frame that did have an outlier is redone the slow way by resolveGate() the next time the host touches the handle
// (which first takes the frame's new landmarks out again: the reference removes the outliers BEFORE it initialises new landmarks
// at the median depth, VIOFilter.cpp:429-443 then :345-391).
int gateSpeculatively(eqf_filter* f, const frame::Meas& m, const double* bearings, long long bearStride, const frame::Lists& perm) {
    const int B = f->B;
    // the permutation the update will use -- the frame's new landmarks appended in measurement order -- is uploaded once, now: the
    // probe reads its first N entries
    frame::Lists permFull = perm;
    for (int b = 0; b < B; ++b)
        if (m.active[b]) frame::forUnmatched(perm[b].data(), int(perm[b].size()), m.n[b], nullptr, [&](int k) { permFull[b].push_back(k); });
    const bool identityPerm = frame::isIdentity(permFull);
    int rc = identityPerm ? EQF_OK : uploadPerm(f, permFull);
    if (!rc) rc = awaitMaskAndClearFlags(f);  // (a redo's k_set_update_ok reads hGate)
    if (!rc) rc = probe(f, bearings, bearStride, !identityPerm, false, true);
    if (!rc) rc = armGate(f, false, m, bearings, bearStride);
    if (rc) return rc;
    f->gate.ids.assign(B, {});
    f->gate.nOld.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        f->gate.ids[b].assign(m.ids[b], m.ids[b] + m.n[b]);
        f->gate.nOld[b] = int(f->ids[b].size());
    }
    f->gate.nb = m.n;
    return EQF_OK;
}

// addNewLandmarks (:345-391) and the update proper (:258-297).  perm: of the state as it is; dropped: the measurement entries the gate
// erased together with their landmark; depthFresh: dDepth2 holds the squared depths of the CURRENT landmark set
int addNewAndUpdate(eqf_filter* f, const frame::Meas& m, const double* bearings, long long bearStride, int* status, frame::Lists& perm,
    const frame::Marks& dropped, bool depthFresh) {
    const int B = f->B, cap = f->cap;
    bool needDepth = false;
    frame::Lists fresh(B);  // measurement indices of new landmarks, in measurement order
    for (int b = 0; b < B; ++b) {
        if (!m.active[b]) continue;
        // (every state id is in the measurement by now: perm marks the measurement entries that have a landmark)
        frame::forUnmatched(perm[b].data(), int(perm[b].size()), m.n[b], dropped[b].data(), [&](int k) { fresh[b].push_back(k); });
        if (!fresh[b].empty()) {
            // (cannot happen: every entry point checks nb <= capacity and strictly ascending ids before any effect)
            if (f->ids[b].size() + fresh[b].size() > (size_t)cap) return EQF_ERR_CAPACITY;
            if (!f->ids[b].empty()) needDepth = true;
        }
    }
    // the host's ids first, then the permutation the update will use (new landmarks at the end, in measurement order): uploaded once, and
    // k_append finds the bearing of the j-th new landmark in it
    std::vector<int> nOldV(B, 0);
    for (int b = 0; b < B; ++b) {
        nOldV[b] = int(f->ids[b].size());
        for (int k : fresh[b]) f->ids[b].push_back(m.ids[b][k]);
    }
    frame::matchPerm(f->ids, m, perm);
    bool anyWork = false;
    int Nmax = 0;
    for (int b = 0; b < B; ++b) {
        if (!m.active[b]) continue;
        if (f->ids[b].empty()) {
            if (status) status[b] = EQF_SKIPPED_NO_BEARINGS;
            continue;
        }
        anyWork = true;
        Nmax = std::max(Nmax, int(f->ids[b].size()));
    }
    const bool identity = frame::isIdentity(perm, &m.active);
    if (anyWork && !identity) {
        int rc = uploadPerm(f, perm);
        if (rc) return rc;
    }
    bool medianLaunch = false;
    if (needDepth) {
        // squared depths of the current estimate on the device (adding landmarks needs no readback); their median is selected by k_append
        // itself, or by a launch of its own for sets too large for that
        // (k_append computes the squared depths itself, round 5: no probe launch in front of it; only sets too large for its LDS take the
        // probe + the selection launch)
        int nmx = 1;
        for (int b = 0; b < B; ++b) {
            if (!fresh[b].empty() && nOldV[b] > kMedianInAppend) medianLaunch = true;
            nmx = std::max(nmx, nOldV[b]);
        }
        int rc = (medianLaunch && !depthFresh) ? probe(f, nullptr, 0, false, false) : EQF_OK;
        if (!rc && medianLaunch) rc = launchMedianDepth(f, nmx);
        if (rc) return rc;
    }
    for (int b = 0; b < B; ++b) {
        if (fresh[b].empty()) continue;
        int rc = launchAppend(f, b, nOldV[b], int(fresh[b].size()), medianLaunch ? f->dDepthSel : nullptr, bearings + (long long)b * bearStride,
            identity ? nullptr : f->dPerm);
        if (rc) return rc;
    }
    if (!anyWork) return EQF_OK;
    return launchUpdate(f, bearings, bearStride, identity ? nullptr : f->dPerm, Nmax);
}

// The frame as separate launches: compaction of the lost landmarks, the gate's probe (and the compaction of what it removed), an append
// launch per filter that gains landmarks, the update.
// Where this path commits: f->ids changes right behind each compaction launch (compactIds) and, for the new landmarks, BEFORE their
// permutation upload and append launches (addNewAndUpdate); status[] there as well.  An error after one of these points leaves the host ahead
// of the device.  That is how it was before this code was split into functions and is kept so on purpose: changing it is a change of
// behaviour for a pull request of its own.
int visionSeparate(eqf_filter* f, const frame::Meas& m, const double* bearings, long long bearStride, int* status, frame::Lists& keep,
    bool anyLost, const frame::Marks* gated) {
    const int B = f->B;
    int rc = flushMeas(f);
    if (!rc && anyLost) rc = compactIds(f, keep);
    if (rc) return rc;
    // ---- matchMeasurementsToState (:211-230): perm[b][i] = measurement index of state landmark i
    frame::Lists perm;
    frame::matchPerm(f->ids, m, perm);
    // ---- removeOutliers (:429-443).  A chord between unit vectors never exceeds 2.
    frame::Marks dropped(B);  // measurement indices erased together with their landmark
    for (int b = 0; b < B; ++b) dropped[b].assign(m.n[b], 0);
    if (gated) dropped = *gated;
    const bool gateOn = !gated && gateCanTrip(f) && maxN(f) > 0;
    bool depthFresh = false;
    if (gateOn && f->gateSpeculative && !f->gate.pending) {  // (lost landmarks are already compacted away)
        rc = gateSpeculatively(f, m, bearings, bearStride, perm);
        if (rc) return rc;
        depthFresh = true;
    } else if (gateOn) {
        const bool identityPerm = frame::isIdentity(perm);
        rc = identityPerm ? EQF_OK : uploadPerm(f, perm);
        if (!rc) rc = probe(f, bearings, bearStride, !identityPerm, true);
        if (rc) return rc;
        for (int b = 0; b < B; ++b)
            if (m.active[b]) recordGate(f, b, int(f->ids[b].size()), true);
        const bool anyOut = frame::gateSync(f->ids, perm, m.active, f->hChord, f->cap, f->gateThr, keep, dropped);
        if (anyOut) {
            rc = compactIds(f, keep);
            if (rc) return rc;
            frame::matchPerm(f->ids, m, perm);
        }
        depthFresh = !anyOut;  // (the probe also left the squared depths -- of the set before any removal)
    }
    return addNewAndUpdate(f, m, bearings, bearStride, status, perm, dropped, depthFresh);
}

// processVisionData after integrateUpToTime: bookkeeping + update.  measIds[b] ascending ids of filter b,
// device bearings at bearings + b*bearStride.  active[b] = integration succeeded && initialised.
// (the index arithmetic of all of it: eqf_frame.hpp)
int visionCore(eqf_filter* f, const std::vector<const int*>& measIds, const std::vector<int>& nb, const double* bearings,
    long long bearStride, const std::vector<char>& active, int* status, const frame::Marks* gated = nullptr) {
    // gated (resolveGate's redo of a frame whose speculative gate tripped): the outliers are known and already removed, (*gated)[b][k] marks
    // their measurement entries -- the gate is not evaluated again
    // innovation statistics: every filter's record starts the vision call with valid = 0; k_innov_stats sets it for the filters whose
    // update runs (a redo of a gated frame only concerns the filters it flags: the others keep what the first pass left)
    if (f->innovStats && !gated) HIPC(hipMemsetAsync(f->dInnov, 0, sizeof(double) * (size_t)(kInnovHead + f->cap) * f->B, f->stream));
    if (!gated) f->report.assign(f->B, {});  // (eqf_get_gate_report describes THIS call from here on)
    const frame::Meas m{measIds, nb, active};
    // ---- removeOldLandmarks (VIOFilter.cpp:393-419): state ids absent from the measurement
    frame::Lists keep;
    const bool anyLost = frame::keepPresent(f->ids, m, keep);
    // The one-launch path is not for a redo itself, filters beyond kEditMax landmarks, a gate whose previous answer is still pending or
    // switched to the synchronous mode, and -- gate armed -- filters so small that losing a landmark could make their two chains equally
    // long (the update's launch shape is chosen from the host's count).
    const bool gateArmed = !gated && gateCanTrip(f) && maxN(f) > 0;
    const bool handleOk = f->deviceEdit && !gated && f->dEdit && (!gateArmed || (f->gateSpeculative && !f->gate.pending));
    const frame::EditChoice e = frame::editEligible(f->ids, keep, m, handleOk, gateArmed, kEditMax, kEditSafeN);
    if (e.ok && (anyLost || e.anyFresh || gateArmed)) return visionOneLaunch(f, m, bearings, bearStride, status, keep, anyLost, gateArmed);
    return visionSeparate(f, m, bearings, bearStride, status, keep, anyLost, gated);
}

// Look at the answer of a speculative outlier gate.  No outlier (the common case): nothing to do.  Otherwise the filters
// that saw one had their update switched off on the device; the frame is redone for them the synchronous way (remove the
// outliers, then update), exactly what a non-speculative call would have done at the time.
int resolveGate(eqf_filter* f) {
    if (!f->gate.pending) return EQF_OK;
    HIPC(hipSetDevice(f->device));
    HIPC(hipEventSynchronize(f->evGate));
    f->gate.pending = false;
    const int B = f->B, cap = f->cap;
    if (f->gate.onDevice) {
        // k_edit took the outliers out before the update ran: the ids follow (kept landmark j of the frame is f->ids[b][j])
        // (flag 2: the outliers left the filter with so few landmarks that k_edit switched the queued update off -- it runs now, shaped for
        // the count the host knows by now; nothing else of the frame is repeated)
        for (int b = 0; b < B; ++b)
            if (f->gate.active[b]) recordGate(f, b, f->gate.nKept[b], f->hGate[b] != 0);
        const frame::DeviceGate d = frame::gateOnDevice(f->ids, f->hGate, f->gate.active, f->gate.nKept, f->hChord, cap, f->gateThr);
        if (!d.deferred) return EQF_OK;
        int rc = launchSetUpdateOk(f);
        if (rc) return rc;
        return launchUpdate(f, f->gate.bearings, f->gate.bearStride, f->dPerm, d.Nmax);
    }
    // The flagged filters: their update did not run, their new landmarks of that frame were appended.  One compaction takes out the
    // outliers -- the probe left every chord in pinned memory: no second probe, no readback -- and the appended landmarks (the redo
    // initialises them again, at the median depth of what is left: the reference's order, VIOFilter.cpp:429-443 then :345-391).
    // (hGate becomes the mask k_set_update_ok reads: only the flagged filters take part in the redo)
    std::vector<char> act;
    frame::Lists keep;
    frame::Marks gated;
    for (int b = 0; b < B; ++b)
        if (f->gate.active[b]) recordGate(f, b, f->gate.nOld[b], f->hGate[b] != 0);
    if (!frame::gateRedo(f->ids, f->hGate, f->gate.active, f->gate.ids, f->gate.nb, f->gate.nOld, f->hChord, cap, f->gateThr, act, keep, gated))
        return EQF_OK;
    int rc = launchSetUpdateOk(f);
    if (!rc) rc = compactIds(f, keep);
    if (rc) return rc;
    std::vector<const int*> mids(B);
    for (int b = 0; b < B; ++b) mids[b] = f->gate.ids[b].data();
    return visionCore(f, mids, f->gate.nb, f->gate.bearings, f->gate.bearStride, act, nullptr, &gated);
}

// Dynamic LDS beyond 64 KB for the kernels of an optional route (see allowUpdateLds): applied once per handle, under the flag `set`, which
// is raised here and nowhere else -- one flag per list of kernels.
struct LdsWant {
    const void* fn;
    int bytes;
};
template <class K>
const void* ldsFn(K* kernel) { return reinterpret_cast<const void*>(kernel); }
int allowRouteLds(bool& set, std::initializer_list<LdsWant> wants) {
    if (set) return EQF_OK;
    for (const LdsWant& w : wants) HIPC(hipFuncSetAttribute(w.fn, hipFuncAttributeMaxDynamicSharedMemorySize, w.bytes));
    set = true;
    return EQF_OK;
}

// ---- the blocked factorisation (eqf_factor.hpp): the one launch loop of every route that factors
// Enqueues A = L L^T of `images` images (grid.y) of order at most mMax each (nb block columns: the one place on the host where an order
// becomes a block-column count for a launch of these kernels), with rhsRows block rows of right-hand side carried along: diag(0) always (it clears the pivot word, also for an empty matrix), then per block column the diagonal block, the panel if a
// block row lies below and the trailing tiles if a block column lies behind.  ldsSet: the handle's flag for the dynamic-LDS attributes
// of this instantiation.
template <class Args>
int enqueueFactor(hipStream_t stream, bool& ldsSet, const Args& a, int images, int mMax, int rhsRows, int* launches = nullptr) {
    const int nb = mMax <= 0 ? 0 : (mMax + kSB - 1) / kSB;
    const int rc = allowRouteLds(ldsSet, {{ldsFn(&k_factor_panel<Args>), kFactorPanelLdsBytes}, {ldsFn(&k_factor_trail<Args>), kFactorTrailLdsBytes}});
    if (rc) return rc;
    int made = 1;
    hipLaunchKernelGGL(k_factor_diag<Args>, dim3(1, images), dim3(256), kLdsFactorBytes, stream, a, 0);
    for (int K = 0; K < nb; ++K) {
        const int t = nb - K - 1;
        made += (K > 0) + (t + rhsRows > 0) + (t > 0);
        if (K > 0) hipLaunchKernelGGL(k_factor_diag<Args>, dim3(1, images), dim3(256), kLdsFactorBytes, stream, a, K);
        if (t + rhsRows > 0) hipLaunchKernelGGL(k_factor_panel<Args>, dim3(t + rhsRows, images), dim3(256), kFactorPanelLdsBytes, stream, a, K, t);
        if (t > 0) hipLaunchKernelGGL(k_factor_trail<Args>, dim3(t * (t + 1) / 2 + rhsRows * t, images), dim3(256), kFactorTrailLdsBytes, stream, a, K, t);
    }
    if (launches) *launches += made;
    return EQF_OK;
}

}  // namespace

extern "C" {

#ifdef EQF_PROP_STAMPS
extern "C" int eqf_debug_prop_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_propStamps), sizeof(long long) * 32) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EQF_STEP64_STAMPS
extern "C" int eqf_debug_step64_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_stamps), sizeof(long long) * 64 * 16) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EQF_CHOL_WG_STAMPS
extern "C" int eqf_debug_chol_wg(long long* t, int* info) {
    if (hipMemcpyFromSymbol(t, HIP_SYMBOL(eqf::g_cholWg), sizeof(long long) * 16 * 256 * 2) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(info, HIP_SYMBOL(eqf::g_cholWgInfo), sizeof(int) * 16 * 256 * 4) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EQF_RES_STAMPS
extern "C" int eqf_debug_res_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_resStamps), sizeof(long long) * 2 * 16 * 16) == hipSuccess ? 0 : -1;
}
#endif
#if defined(EQF_RES_STAMPS) && defined(EQF_F64_STAMPS)
extern "C" int eqf_debug_res_f64_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_resF64), sizeof(long long) * 2 * 16 * 128) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EQF_WAIT_STATS
extern "C" int eqf_debug_wait_stats(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_waitStats), sizeof(unsigned long long) * 48) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[48] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(eqf::g_waitStats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef EQF_PREP_STAMPS
extern "C" int eqf_debug_prep_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_prepStamps), sizeof(long long) * 1024) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EQF_BURST_STAMPS
extern "C" int eqf_debug_ring_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_ringStamps), sizeof(long long) * 256) == hipSuccess ? 0 : -1;
}
extern "C" int eqf_debug_burst_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(eqf::g_burstStamps), sizeof(long long) * 8 * 20 * 4) == hipSuccess ? 0 : -1;
}
#endif
const char* eqf_version(void) { return "eqf_vio_amd 0.1 (gfx950)"; }

// sha256 of the sources this library was built from (csrc/Makefile: eqf_build_id.inc)
const char* eqf_build_info(void) {
    return "src_sha256="
#include "eqf_build_id.inc"
        ;
}

void eqf_settings_default(eqf_settings* s) {  // VIOFilterSettings.h:29-50
    std::memset(s, 0, sizeof(*s));
    s->biasOmegaProcessVariance = 0.001;
    s->biasAccelProcessVariance = 0.001;
    s->gravityProcessVariance = 0.001;
    s->velocityProcessVariance = 0.001;
    s->pointProcessVariance = 0.001;
    s->velOmegaVariance = 0.1;
    s->velAccelVariance = 0.1;
    s->measurementVariance = 0.1;
    s->initialGravityVariance = 1.0;
    s->initialVelocityVariance = 1.0;
    s->initialPointVariance = 1.0;
    s->initialBiasOmegaVariance = 1.0;
    s->initialBiasAccelVariance = 1.0;
    s->initialSceneDepth = 1.0;
    s->outlierThreshold = 0.01;
    s->useInnovationLift = 1;
    s->useDiscreteInnovationLift = 1;
    s->useDiscreteVelocityLift = 1;
    s->fastRiccati = 0;
    s->cameraOffset_q[0] = 1.0;
}

// camera-offset constants, same formulas as on the device (eqf_math.hpp is host+device)
static void setCameraConstants(Params& p) {
    const quat cq = quat{p.camq[0], p.camq[1], p.camq[2], p.camq[3]};
    const se3 camI = se3inv(se3{cq, mk3(p.camx[0], p.camx[1], p.camx[2])});
    const m33 RIC = q2m(cq), RICt = q2m(qinv(cq)), RcI = q2m(camI.q);
    for (int i = 0; i < 9; ++i) {
        p.RIC[i] = RIC.a[i];
        p.RICt[i] = RICt.a[i];
        p.RcamI[i] = RcI.a[i];
    }
    p.camIq[0] = camI.q.w; p.camIq[1] = camI.q.x; p.camIq[2] = camI.q.y; p.camIq[3] = camI.q.z;
    p.camIx[0] = camI.x.x; p.camIx[1] = camI.x.y; p.camIx[2] = camI.x.z;
}

int eqf_create(const eqf_settings* settings, int capacity_landmarks, int batch, int device, int precision, eqf_filter** out) {
    if (!settings || !out || capacity_landmarks < 1 || batch < 1) return EQF_ERR_INVALID;
    if (precision != EQF_PRECISION_F64 && precision != EQF_PRECISION_F32) return EQF_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return EQF_ERR_NO_DEVICE;
    HIPC(hipSetDevice(device));
    eqf_filter* f = new eqf_filter();
    f->B = batch;
    f->cap = capacity_landmarks;
    f->device = device;
    f->precision = precision;
    f->esz = precision == EQF_PRECISION_F32 ? 4 : 8;
    f->set = *settings;
    f->gateThr = settings->outlierThreshold;
    Params& p = f->prm;
    p.biasOmegaProcessVariance = settings->biasOmegaProcessVariance;
    p.biasAccelProcessVariance = settings->biasAccelProcessVariance;
    p.gravityProcessVariance = settings->gravityProcessVariance;
    p.velocityProcessVariance = settings->velocityProcessVariance;
    p.pointProcessVariance = settings->pointProcessVariance;
    p.velOmegaVariance = settings->velOmegaVariance;
    p.velAccelVariance = settings->velAccelVariance;
    p.measurementVariance = settings->measurementVariance;
    p.initialPointVariance = settings->initialPointVariance;
    std::memcpy(p.camq, settings->cameraOffset_q, sizeof(p.camq));
    std::memcpy(p.camx, settings->cameraOffset_x, sizeof(p.camx));
    p.useInnovationLift = settings->useInnovationLift;
    p.useDiscreteInnovationLift = settings->useDiscreteInnovationLift;
    p.useDiscreteVelocityLift = settings->useDiscreteVelocityLift;
    setCameraConstants(p);

    const int B = batch, cap = f->cap;
    f->nTot = kLm0 + 3 * cap;
    f->ld = roundUp(f->nTot, 16);
    f->sigmaStride = (long long)f->nTot * f->ld;
    const int mpC = roundUp(2 * cap, kSB), nepC = roundUp(eDim(cap), kSB), ycC = roundUp(yCols(cap), kSB);
    f->ldS = mpC; f->ldY = ycC; f->ldE = nepC; f->ldZ = kSB;
    f->strideS = (long long)mpC * mpC; f->strideY = (long long)mpC * ycC;
    f->strideE = (long long)nepC * nepC; f->strideZ = (long long)nepC * kSB;
    const clone::SmallLayout sm = cloneSmall(f);  // (doubles per filter of the small state's arrays)
    const frame::ImageLayout fi = frameImage(f);
    int rc = EQF_OK;
    auto chk = [&](int r) { if (r && !rc) rc = r; };
    if (hipStreamCreateWithFlags(f->stream.put(), hipStreamNonBlocking) != hipSuccess) rc = EQF_ERR_HIP;
    for (int q = 0; q < 2 && !rc; ++q) {
        chk(dmalloc(f->Sigma[q], (size_t)f->sigmaStride * B, f->esz));
        chk(dmalloc(f->g[q], B));
        chk(dmalloc(f->Q[q], sm.qCount() * B));
    }
    chk(dmalloc(f->p0, sm.p0Count() * B));
    chk(dmalloc(f->lmc, (size_t)15 * cap * B));
    f->strideDS = std::max<long long>(f->strideS, (long long)(mpC / kSB) * kDRec);
    f->strideDE = std::max<long long>(f->strideE, (long long)(nepC / kSB) * kDRec);
    chk(dmalloc(f->SA, f->strideS * B)); chk(dmalloc(f->SL, f->strideDS * B));
    chk(dmalloc(f->YW, f->strideY * B)); chk(dmalloc(f->YO, f->strideY * B));
    chk(dmalloc(f->EA, f->strideE * B)); chk(dmalloc(f->EL, f->strideDE * B));
    chk(dmalloc(f->ZW, f->strideZ * B)); chk(dmalloc(f->ZO, f->strideZ * B));
    chk(dmalloc(f->dbgDelta, sm.deltaCount() * B));
    chk(dmalloc(f->dbgGamma, sm.gammaCount() * B));
    chk(dmalloc(f->dbgGammaTot, sm.gammaTotCount() * B));
    chk(dmalloc(f->red, (size_t)256 * B));
    chk(dmalloc(f->errflag, 1));
    chk(dmalloc(f->dMap, (size_t)cap * B + B)); if (!rc) f->dNewN = f->dMap + (size_t)cap * B;  /* (one copy brings both) */ chk(dmalloc(f->dPerm, (size_t)cap * B));
    chk(dmalloc(f->dChord, (size_t)cap * B)); chk(dmalloc(f->dDepth2, (size_t)cap * B));
    chk(dmalloc(f->dScratch, (size_t)kLmRec * cap * B)); chk(dmalloc(f->dMeas, fi.doubles()));  /* (k_edit's image behind the bearings: one copy brings both) */
    chk(dmalloc(f->dOut, (size_t)f->nTot * f->nTot + 16));
    chk(dmalloc(f->dRing, (size_t)kRing * B));
    chk(dmalloc(f->dBlk, (size_t)kBlkRec * cap * B, f->esz));
    chk(dmalloc(f->dBlkCommon, B));
    chk(dmalloc(f->dColRec, (size_t)kBurstMax * burstRecStep((long long)kColRec * cap) * B, f->esz));
    chk(dmalloc(f->dRowRec, (size_t)kBurstMax * burstRecStep((long long)kBlkRec * cap) * B, f->esz));
    chk(dmalloc(f->dSteps, (size_t)kBurstMax * B));
    f->nBuildCap = ((cap + 3) / 4 + 63) / 64 * 64 + 1088;  // stride of a replica: > 4 KB, not a multiple of it
    chk(dmalloc(f->dBuildFlags, (size_t)f->nBuildCap * kFlagReplicas * B));
    if (!rc && hipMemset(f->dBuildFlags, 0, sizeof(int) * f->nBuildCap * kFlagReplicas * B) != hipSuccess) rc = EQF_ERR_HIP;
    if (const char* e = std::getenv("EQF_BURST_ROWS")) f->burstRows = (std::atoi(e) == 1 || std::atoi(e) == 2 || std::atoi(e) == 4) ? std::atoi(e) : 0;
    if (const char* e = std::getenv("EQF_IMU_BURST")) f->burstMax = std::max(0, std::min(kBurstMax, std::atoi(e)));
    if (const char* e = std::getenv("EQF_SPLIT_PROPAGATE")) f->splitPropagate = std::atoi(e);
    if (const char* e = std::getenv("EQF_CHOL_SPLIT")) f->cholSplit = std::atoi(e);
    if (const char* e = std::getenv("EQF_CHOL_RESIDENT")) f->cholResident = std::atoi(e);
    if (const char* e = std::getenv("EQF_RES_FOLD_PREP")) f->resFoldPrep = std::atoi(e);
    if (const char* e = std::getenv("EQF_BURST_FUSED")) f->burstFused = std::atoi(e);
    {
        hipDeviceProp_t prop;
        if (!rc && hipGetDeviceProperties(&prop, device) != hipSuccess) rc = EQF_ERR_HIP;
        if (!rc) f->numCUs = prop.multiProcessorCount;
        f->nbCap = std::max(mpC, nepC) / kSB;
        f->wtCap = ycC / kSB;
        // the resident kernel's role table holds one workgroup per 64 x 64 tile; its flag / partial-sum buffers are allocated up to 200 k
        // roles in the batch (one filter of N = 4000: 71 k), beyond that the per-column launches run
        const long long maxRoles = (long long)(f->nbCap + 1) * f->nbCap + (long long)f->wtCap * f->nbCap;
        if (!rc && maxRoles * B <= 200000) {  // (N = 4000: 71 k roles)
            chk(dmalloc(f->dReadyA, (size_t)2 * f->nbCap * f->nbCap * B));
            chk(dmalloc(f->dReadyY, (size_t)2 * f->nbCap * f->wtCap * B));
            chk(dmalloc(f->dResCounters, (size_t)4 * B));
            chk(dmalloc(f->dTicket, (size_t)32 * B));  // (one counter per filter, a 128-byte line each)
            if (!rc && hipMemset(f->dTicket, 0, sizeof(unsigned) * 32 * B) != hipSuccess) rc = EQF_ERR_HIP;
            chk(dmalloc(f->dStageFlags, (size_t)2 * f->nbCap * 4 * B));
            if (!rc && hipMemset(f->dStageFlags, 0, sizeof(int) * 2 * f->nbCap * 4 * B) != hipSuccess) rc = EQF_ERR_HIP;
            f->nPrepCap = (mpC / 2 + 3) / 1 + nepC / kNB + 8;  // (landmark workgroups carry >= 1 wave each; Z-row workgroups of kNB rows)
            chk(dmalloc(f->dPrepFlags, (size_t)f->nPrepCap * B));
            if (!rc && hipMemset(f->dPrepFlags, 0, sizeof(int) * f->nPrepCap * B) != hipSuccess) rc = EQF_ERR_HIP;
            chk(dmalloc(f->dGammaPart, (size_t)f->nbCap * ycC * B));
            chk(dmalloc(f->dG11Part, (size_t)f->nbCap * 128 * B));
            if (!rc && (hipMemset(f->dReadyA, 0, sizeof(int) * 2 * f->nbCap * f->nbCap * B) != hipSuccess ||
                        hipMemset(f->dReadyY, 0, sizeof(int) * 2 * f->nbCap * f->wtCap * B) != hipSuccess ||
                        hipMemset(f->dResCounters, 0, sizeof(int) * 4 * B) != hipSuccess))
                rc = EQF_ERR_HIP;
        }
    }
    f->flagStride = std::max(mpC, nepC) / kSB + 1;
    chk(dmalloc(f->dFlags, (size_t)2 * f->flagStride * B));
    if (!rc && hipMemset(f->dFlags, 0, sizeof(int) * 2 * f->flagStride * B) != hipSuccess) rc = EQF_ERR_HIP;
    if (const char* e = std::getenv("EQF_GATE_SPECULATIVE")) f->gateSpeculative = std::atoi(e);
    chk(stageInit(f, f->stMap, (size_t)cap * B + B)); chk(stageInit(f, f->stPerm, (size_t)cap * B));
    chk(stageInit(f, f->stEdit, fi.editInts())); chk(dmalloc(f->dEdit, fi.editInts())); chk(dmalloc(f->dEditBar, (size_t)4 * B));
    if (!rc && hipMemset(f->dEditBar, 0, sizeof(int) * 4 * B) != hipSuccess) rc = EQF_ERR_HIP;
    chk(hmalloc(f->hChord, (size_t)cap * B)); chk(dmalloc(f->dDepthSel, B));
    chk(hmalloc(f->hGate, B)); chk(dmalloc(f->dMask, B));
    chk(eventInit(f, f->evGate)); chk(eventInit(f, f->evMask)); chk(eventInit(f, f->evMeas));
    chk(hmalloc(f->hMeas, fi.doubles())); chk(hmalloc(f->hOut, (size_t)f->nTot * f->nTot + 16));
    chk(hmalloc(f->hRing, (size_t)kRing * B));
    for (auto& e : f->evRing) chk(eventInit(f, e));
    if (!rc) rc = initState(f);
    if (rc) {
        delete f;  // (the device is current: every owner frees what it got, the stream last)
        return rc;
    }
    *out = f;
    return EQF_OK;
}

void eqf_destroy(eqf_filter* f) {
    if (!f) return;
    hipSetDevice(f->device);
    if (f->stream) hipStreamSynchronize(f->stream);
    delete f;
}

int eqf_reset(eqf_filter* f) {
    if (!f) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    HIPC(hipStreamSynchronize(f->stream));
    // (no vision call has been made on the fresh state: the innovation statistics of the old one are not valid any more)
    if (f->dInnov) HIPC(hipMemsetAsync(f->dInnov, 0, sizeof(double) * (size_t)(kInnovHead + f->cap) * f->B, f->stream));
    return initState(f);
}

int eqf_synchronize(eqf_filter* f) {
    if (!f) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipStreamSynchronize(f->stream));
    return EQF_OK;
}

int eqf_process_imu(eqf_filter* f, const double* stamps, const double* omega, const double* accel, int* status) {
    if (!f || !stamps || !omega || !accel) return EQF_ERR_INVALID;
    const bool burst = burstEligible(f, true);
    if (!(burst && f->B == 1 && f->burst.kind != 1)) GATE(f);  // (a queued call settles nothing: it is only recorded)
    HIPC(hipSetDevice(f->device));
    std::vector<ImuRec> recs(f->B);
    for (int b = 0; b < f->B; ++b) {
        recs[b].stamp = stamps[b];
        for (int i = 0; i < 3; ++i) {
            recs[b].w[i] = omega[3 * b + i];
            recs[b].a[i] = accel[3 * b + i];
        }
        recs[b].pad_ = 0;
    }
    if (burst && f->B == 1) {
        // one filter: queue the record; the burst is launched when it is full or when anything else touches the handle
        auto& q = f->burst;
        q.kind = 2;
        q.inl[q.cnt++] = recs[0];
        mirrorStep(f, stamps, true, status);
        if (q.cnt >= std::min(f->burstMax, kBurstMax - 1) || !allDevInit(f)) {
            GATE(f);
        }
        return EQF_OK;
    }
    const ImuRec* dev = nullptr;
    int slot = -1;
    int rc = stageRecs(f, recs.data(), &dev, &slot);
    if (rc) return rc;
    if (burst) {
        rc = launchBurst(f, 1, dev, 0, nullptr, false, nullptr);
        if (!rc) mirrorStep(f, stamps, true, status);
    } else {
        rc = launchPropagate(f, dev, recs[0], stamps, true, !f->set.fastRiccati, status);
    }
    if (rc) return rc;
    return releaseSlot(f, slot);
}

int eqf_process_vision(eqf_filter* f, const double* stamps, const int* nb, const int* ids, const double* bearings, int stride,
    int* status) {
    if (!f || !stamps || !nb || (!ids && stride > 0) || (!bearings && stride > 0)) return EQF_ERR_INVALID;
    HIPC(hipSetDevice(f->device));
    const int B = f->B, cap = f->cap;
    // Argument errors are reported before ANY effect (nothing enqueued, no time advanced).  After removeOldLandmarks the
    // state's ids are a subset of the measurement's and addNewLandmarks appends the rest, so nb <= capacity is the whole
    // capacity condition of the call (the reference grows Sigma on demand instead, VIOFilter.cpp:386).  Ids must be strictly
    // ascending: the reference asserts is_sorted (VIOFilter.cpp:239-240) and a duplicate id would map two bearings to one
    // landmark / append one landmark twice.
    for (int b = 0; b < B; ++b) {
        if (nb[b] < 0 || nb[b] > stride) return EQF_ERR_INVALID;
        if (nb[b] > cap) return EQF_ERR_CAPACITY;
        for (int k = 1; k < nb[b]; ++k)
            if (ids[(size_t)b * stride + k] <= ids[(size_t)b * stride + k - 1]) return EQF_ERR_UNSORTED;
    }
    {
        const int grc = burstEligible(f, false) ? resolveGate(f) : (resolveGate(f) || flushBurst(f));
        if (grc) return grc;
    }
    // integrateUpToTime(measurement.stamp) (VIOFilter.cpp:234)
    std::vector<ImuRec> recs(B);
    for (int b = 0; b < B; ++b) {
        std::memset(&recs[b], 0, sizeof(ImuRec));
        recs[b].stamp = stamps[b];
    }
    const ImuRec* dev = nullptr;
    int slot = -1;
    int rc = stageRecs(f, recs.data(), &dev, &slot);
    if (rc) return rc;
    std::vector<int> st(B, EQF_OK);
    if (burstEligible(f, false)) {
        rc = flushBurstWith(f, true, dev, &recs[0]);
        if (!rc) mirrorStep(f, stamps, false, st.data());
    } else {
        rc = launchPropagate(f, dev, recs[0], stamps, false, true, st.data());
    }
    if (status) std::copy(st.begin(), st.end(), status);
    if (rc) return rc;
    rc = releaseSlot(f, slot);
    if (rc) return rc;
    // bearings -> device
    HIPC(hipEventSynchronize(f->evMeas));
    std::vector<const int*> mids(B);
    std::vector<int> nbv(nb, nb + B);
    std::vector<char> active(B);
    const size_t bearStride = frameImage(f).bearingStride();
    for (int b = 0; b < B; ++b) {
        std::memcpy(f->hMeas + (size_t)b * bearStride, bearings + (size_t)b * stride * 3, sizeof(double) * 3 * nb[b]);
        mids[b] = ids + (size_t)b * stride;
        active[b] = st[b] == EQF_OK;
    }
    f->measPending = true;
    rc = visionCore(f, mids, nbv, f->dMeas, (long long)bearStride, active, st.data());
    if (flushMeas(f)) return EQF_ERR_HIP;  // (visionCore left before it needed them)
    if (status) std::copy(st.begin(), st.end(), status);
    return rc;
}

int eqf_stream_upload(eqf_filter* f, int K, const double* imu, int F, const double* vstamps, int nbear, const int* ids,
    const double* bearings) {
    if (!f || K < 0 || F < 0 || nbear < 0 || nbear > f->cap) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    HIPC(hipStreamSynchronize(f->stream));
    const int B = f->B;
    for (int k = 1; k < nbear; ++k)
        if (ids[k] <= ids[k - 1]) return EQF_ERR_UNSORTED;  // strictly ascending, as in eqf_process_vision
    f->sImu.reset(); f->sVis.reset(); f->sBear.reset();
    std::vector<ImuRec> ri((size_t)K * B), rv((size_t)F * B);
    f->hImuStamp.resize((size_t)K * B);
    f->hVisStamp.resize((size_t)F * B);
    for (size_t e = 0; e < (size_t)K * B; ++e) {
        const double* s = imu + 7 * e;
        ri[e].stamp = s[0];
        for (int i = 0; i < 3; ++i) {
            ri[e].w[i] = s[1 + i];
            ri[e].a[i] = s[4 + i];
        }
        ri[e].pad_ = 0;
        f->hImuStamp[e] = s[0];
    }
    for (size_t e = 0; e < (size_t)F * B; ++e) {
        std::memset(&rv[e], 0, sizeof(ImuRec));
        rv[e].stamp = vstamps[e];
        f->hVisStamp[e] = vstamps[e];
    }
    int rc = dmalloc(f->sImu, ri.size());
    if (!rc) rc = dmalloc(f->sVis, rv.size());
    if (!rc) rc = dmalloc(f->sBear, (size_t)F * B * nbear * 3);
    if (rc) return rc;
    HIPC(hipMemcpy(f->sImu, ri.data(), sizeof(ImuRec) * ri.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(f->sVis, rv.data(), sizeof(ImuRec) * rv.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(f->sBear, bearings, sizeof(double) * (size_t)F * B * nbear * 3, hipMemcpyHostToDevice));
    f->sK = K; f->sF = F; f->sNb = nbear;
    f->sIds.assign(ids, ids + nbear);
    return EQF_OK;
}

int eqf_stream_imu(eqf_filter* f, int k) {
    if (!f || k < 0 || k >= f->sK) return EQF_ERR_INVALID;
    if (burstEligible(f, true)) {
        auto& q = f->burst;
        if (q.kind && !(q.kind == 1 && k == q.k0 + q.cnt)) GATE(f);  // not the record after the queued ones: launch those first
        if (!q.kind) {
            q.kind = 1;
            q.k0 = k;
            q.cnt = 0;
        }
        ++q.cnt;
        mirrorStep(f, f->hImuStamp.data() + (size_t)k * f->B, true, nullptr);
        if (q.cnt >= std::min(f->burstMax, kBurstMax - 1) || !allDevInit(f)) {
            GATE(f);
        }
        return EQF_OK;
    }
    GATE(f);
    ImuRec dummy{};
    return launchPropagate(f, f->sImu + (size_t)k * f->B, dummy, f->hImuStamp.data() + (size_t)k * f->B, true, !f->set.fastRiccati, nullptr);
}

int eqf_stream_vision(eqf_filter* f, int fr) {
    if (!f || fr < 0 || fr >= f->sF) return EQF_ERR_INVALID;
    const int B = f->B;
    ImuRec dummy{};
    std::vector<int> st(B, EQF_OK);
    HIPC(hipSetDevice(f->device));
    int rc = resolveGate(f);
    if (rc) return rc;
    if (burstEligible(f, false)) {
        // the queued IMU steps and this call's integrateUpToTime leave as one burst
        rc = flushBurstWith(f, true, f->sVis + (size_t)fr * B, nullptr);
        if (!rc) mirrorStep(f, f->hVisStamp.data() + (size_t)fr * B, false, st.data());
    } else {
        rc = flushBurst(f);
        if (!rc) rc = launchPropagate(f, f->sVis + (size_t)fr * B, dummy, f->hVisStamp.data() + (size_t)fr * B, false, true, st.data());
    }
    if (rc) return rc;
    std::vector<const int*> mids(B, f->sIds.data());
    std::vector<int> nbv(B, f->sNb);
    std::vector<char> active(B);
    for (int b = 0; b < B; ++b) active[b] = st[b] == EQF_OK;
    return visionCore(f, mids, nbv, f->sBear + (size_t)fr * B * f->sNb * 3, (long long)f->sNb * 3, active, st.data());
}

int eqf_get_time(eqf_filter* f, double* t) {
    if (!f || !t) return EQF_ERR_INVALID;
    std::copy(f->curTime.begin(), f->curTime.end(), t);
    return EQF_OK;
}

int eqf_num_landmarks(eqf_filter* f, int b) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    if (resolveGate(f)) return EQF_ERR_HIP;
    return int(f->ids[b].size());
}

int eqf_get_ids(eqf_filter* f, int b, int* ids) {
    if (!f || b < 0 || b >= f->B || !ids) return EQF_ERR_INVALID;
    GATE(f);
    std::copy(f->ids[b].begin(), f->ids[b].end(), ids);
    return EQF_OK;
}

int eqf_get_state_estimate(eqf_filter* f, int b, double* pose_q, double* pose_x, double* velocity, double* p) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    const int N = int(f->ids[b].size());
    hipLaunchKernelGGL(k_state_estimate, dim3((N + 255) / 256 + 1), dim3(256), 0, f->stream, f->g[f->pG], b, f->p0, f->Q[f->pG], f->cap, f->dOut);
    HIPC(hipMemcpyAsync(f->hOut, f->dOut, sizeof(double) * (10 + 3 * N), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    if (pose_q) std::copy(f->hOut.get(), f->hOut + 4, pose_q);
    if (pose_x) std::copy(f->hOut + 4, f->hOut + 7, pose_x);
    if (velocity) std::copy(f->hOut + 7, f->hOut + 10, velocity);
    if (p) std::copy(f->hOut + 10, f->hOut + 10 + 3 * N, p);
    return EQF_OK;
}

static int fetchGlob(eqf_filter* f, int b, Glob* g) {
    HIPC(hipSetDevice(f->device));
    HIPC(hipStreamSynchronize(f->stream));
    HIPC(hipMemcpy(g, f->g[f->pG] + b, sizeof(Glob), hipMemcpyDeviceToHost));
    return EQF_OK;
}

int eqf_get_origin(eqf_filter* f, int b, double* pose_q, double* pose_x, double* velocity, double* p) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    GATE(f);
    Glob g;
    int rc = fetchGlob(f, b, &g);
    if (rc) return rc;
    if (pose_q) std::copy(g.P0q, g.P0q + 4, pose_q);
    if (pose_x) std::copy(g.P0x, g.P0x + 3, pose_x);
    if (velocity) std::copy(g.v0, g.v0 + 3, velocity);
    if (p) {
        const int N = int(f->ids[b].size()), cap = f->cap;
        std::vector<double> tmp((size_t)3 * cap);
        HIPC(hipMemcpy(tmp.data(), f->p0 + (size_t)b * 3 * cap, sizeof(double) * 3 * cap, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
            for (int c = 0; c < 3; ++c) p[3 * i + c] = tmp[(size_t)c * cap + i];
    }
    return EQF_OK;
}

int eqf_get_group(eqf_filter* f, int b, double* A_q, double* A_x, double* w, double* Q_q, double* Q_a) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    GATE(f);
    Glob g;
    int rc = fetchGlob(f, b, &g);
    if (rc) return rc;
    if (A_q) std::copy(g.Aq, g.Aq + 4, A_q);
    if (A_x) std::copy(g.Ax, g.Ax + 3, A_x);
    if (w) std::copy(g.w, g.w + 3, w);
    if (Q_q || Q_a) {
        const int N = int(f->ids[b].size()), cap = f->cap;
        std::vector<double> tmp((size_t)5 * cap);
        HIPC(hipMemcpy(tmp.data(), f->Q[f->pG] + (size_t)b * 5 * cap, sizeof(double) * 5 * cap, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i) {
            if (Q_q)
                for (int c = 0; c < 4; ++c) Q_q[4 * i + c] = tmp[(size_t)c * cap + i];
            if (Q_a) Q_a[i] = tmp[(size_t)4 * cap + i];
        }
    }
    return EQF_OK;
}

int eqf_get_bias(eqf_filter* f, int b, double* bias6) {
    if (!f || b < 0 || b >= f->B || !bias6) return EQF_ERR_INVALID;
    GATE(f);
    Glob g;
    int rc = fetchGlob(f, b, &g);
    if (rc) return rc;
    std::copy(g.bias, g.bias + 6, bias6);
    return EQF_OK;
}

int eqf_get_sigma(eqf_filter* f, int b, double* dst, int ld) {
    if (!f || b < 0 || b >= f->B || !dst) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    const int n = kBase + 3 * int(f->ids[b].size());
    if (ld < n) return EQF_ERR_INVALID;
    const dim3 grid((n + 255) / 256, n);
    if (f->precision == EQF_PRECISION_F32)
        hipLaunchKernelGGL(k_sigma_export<float>, grid, dim3(256), 0, f->stream,
            static_cast<const float*>(f->Sigma[f->pS]) + (long long)b * f->sigmaStride, f->ld, n, f->dOut, n);
    else
        hipLaunchKernelGGL(k_sigma_export<double>, grid, dim3(256), 0, f->stream,
            static_cast<const double*>(f->Sigma[f->pS]) + (long long)b * f->sigmaStride, f->ld, n, f->dOut, n);
    HIPC(hipMemcpyAsync(f->hOut, f->dOut, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    for (int r = 0; r < n; ++r) std::copy(f->hOut + (size_t)r * n, f->hOut + (size_t)(r + 1) * n, dst + (size_t)r * ld);
    return EQF_OK;
}

// The J blocks of filters [b0, b0 + count) (k_local_jacobian) behind whatever the stream holds; with sigmaToo the image of Sigma in the
// coordinates of the estimate as well (k_sigma_local).  The buffers are allocated on first use: a failed allocation is EQF_ERR_HIP and
// leaves the handle as it was.
static int launchLocal(eqf_filter* f, int b0, int count, bool sigmaToo) {
    {
        const workspace::Want w[] = {want(f->dJac, sizeof(double) * size_t(jacStride(f->cap)) * f->B), sigmaLocWant(f, sigmaToo)};
        const int rc = reserveSlots(f, w);
        if (rc) return rc;
    }
    int nMax = 0;
    for (int b = b0; b < b0 + count; ++b) nMax = std::max(nMax, int(f->ids[b].size()));
    LocalArgs a{};
    a.g = f->g[f->pG]; a.Q = f->Q[f->pG]; a.cap = f->cap; a.b0 = b0; a.jac = f->dJac;
    a.Sin = static_cast<const double*>(f->Sigma[f->pS]); a.Sout = f->dSigmaLoc; a.ld = f->ld; a.sigmaStride = f->sigmaStride;
    const int strips = std::max(1, (nMax + 255) / 256);
    hipLaunchKernelGGL(k_local_jacobian, dim3(strips, count), dim3(256), 0, f->stream, a);
    if (sigmaToo)
        hipLaunchKernelGGL(k_sigma_local, dim3(strips, std::max(1, (nMax + kLocalRows - 1) / kLocalRows), count), dim3(256), 0, f->stream, a);
    HIPC(hipGetLastError());
    return EQF_OK;
}
static LocalArgs localArgs(eqf_filter* f, int b) {
    LocalArgs a{};
    a.g = f->g[f->pG]; a.Q = f->Q[f->pG]; a.cap = f->cap; a.b0 = b; a.jac = f->dJac;
    a.Sin = static_cast<const double*>(f->Sigma[f->pS]); a.Sout = f->dSigmaLoc; a.ld = f->ld; a.sigmaStride = f->sigmaStride;
    return a;
}

int eqf_get_sigma_local(eqf_filter* f, int b, double* dst, int ld) {
    if (!f || b < 0 || b >= f->B || !dst) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int n = kBase + 3 * int(f->ids[b].size());
    if (ld < n) return EQF_ERR_INVALID;
    int rc = launchLocal(f, b, 1, true);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sigma_export<double>, dim3((n + 255) / 256, n), dim3(256), 0, f->stream, f->dSigmaLoc + (long long)b * f->sigmaStride,
        f->ld, n, f->dOut, n);
    HIPC(hipMemcpyAsync(f->hOut, f->dOut, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, f->stream));
    double head[kJacHead];
    HIPC(hipMemcpyAsync(head, f->dJac + (long long)b * jacStride(f->cap), sizeof(head), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    if (head[13] != 0.0) return EQF_ERR_NUMERIC;
    for (int r = 0; r < n; ++r) std::copy(f->hOut + (size_t)r * n, f->hOut + (size_t)(r + 1) * n, dst + (size_t)r * ld);
    return EQF_OK;
}

int eqf_get_marginals(eqf_filter* f, int b, int local, double* base, double* lm) {
    if (!f || b < 0 || b >= f->B || !base || (local != 0 && local != 1)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int N = int(f->ids[b].size());
    if (N > 0 && !lm) return EQF_ERR_INVALID;
    int rc = launchLocal(f, b, 1, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_marginals, dim3(std::max(1, (N + 255) / 256)), dim3(256), 0, f->stream, localArgs(f, b), local, f->dOut);
    HIPC(hipMemcpyAsync(f->hOut, f->dOut, sizeof(double) * (121 + (size_t)9 * N), hipMemcpyDeviceToHost, f->stream));
    double head[kJacHead];
    HIPC(hipMemcpyAsync(head, f->dJac + (long long)b * jacStride(f->cap), sizeof(head), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    if (local && head[13] != 0.0) return EQF_ERR_NUMERIC;
    std::copy(f->hOut.get(), f->hOut + 121, base);
    if (N > 0) std::copy(f->hOut + 121, f->hOut + 121 + (size_t)9 * N, lm);
    return EQF_OK;
}

int eqf_get_local_jacobian(eqf_filter* f, int b, double* G, double* RAt, double* lmJ) {
    if (!f || b < 0 || b >= f->B || !G || !RAt) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int N = int(f->ids[b].size());
    if (N > 0 && !lmJ) return EQF_ERR_INVALID;
    int rc = launchLocal(f, b, 1, false);
    if (rc) return rc;
    HIPC(hipMemcpyAsync(f->hOut, f->dJac + (long long)b * jacStride(f->cap), sizeof(double) * (kJacHead + (size_t)9 * N), hipMemcpyDeviceToHost,
        f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    if (f->hOut[13] != 0.0) return EQF_ERR_NUMERIC;
    std::copy(f->hOut.get(), f->hOut + 4, G);
    std::copy(f->hOut + 4, f->hOut + 13, RAt);
    if (N > 0) std::copy(f->hOut + kJacHead, f->hOut + kJacHead + (size_t)9 * N, lmJ);
    return EQF_OK;
}

// eqf_forecast's workspace, from capacity and batch
static int forecastWorkspace(eqf_filter* f) {
    const size_t nImg = sizeof(double) * forecast::imageCapacityDoubles(f->B), nRec = sizeof(double) * forecast::recDoubles(f->B),
                 nOut = sizeof(double) * forecast::outStride(f->cap) * f->B;
    const workspace::Want w[] = {want(f->fc.hImu, nImg), want(f->fc.dImu, nImg), want(f->fc.rec, nRec), want(f->fc.dOut, nOut), want(f->fc.hOut, nOut)};
    return reserveSlots(f, w);
}

int eqf_forecast(eqf_filter* f, int K, const double* imu, const double* t1, int local, int stride, const eqf_forecast_out* out, int* status) {
    namespace fc = forecast;
    if (!fc::headArgsOk(f, out, K, imu, local, stride)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64 || f->set.fastRiccati) return EQF_ERR_UNSUPPORTED;
    const int B = f->B, cap = f->cap;
    if (!fc::stampsOk(K, imu, t1, B)) return EQF_ERR_INVALID;
    GATE(f);
    const std::vector<int> N = landmarkCounts(f);
    const fc::Wants wants{out->p != nullptr, out->bearing != nullptr, out->lm != nullptr, out->S != nullptr, out->ycov != nullptr};
    if (!fc::strideOk(wants, stride, B, N.data())) return EQF_ERR_INVALID;
    int rc = forecastWorkspace(f);
    if (rc) return rc;
    const int nSteps = fc::steps(K, t1 != nullptr);
    double* img = reinterpret_cast<double*>(f->fc.hImu.get());
    for (int k = 0; k < K; ++k)
        for (int b = 0; b < B; ++b) fc::packSample(imu + ((size_t)k * B + b) * 7, img + fc::imageIndex(k, b, B));
    if (t1)
        for (int b = 0; b < B; ++b) fc::packStamp(t1[b], img + fc::imageIndex(K, b, B));
    if (nSteps > 0)
        HIPC(hipMemcpyAsync(f->fc.dImu, f->fc.hImu, sizeof(double) * fc::imageDoubles(K, t1 != nullptr, B), hipMemcpyHostToDevice, f->stream));
    FcArgs a{};
    a.g = f->g[f->pG]; a.p0 = f->p0; a.Q = f->Q[f->pG]; a.lmc = f->lmc;
    a.Sin = static_cast<const double*>(f->Sigma[f->pS]); a.sigmaStride = f->sigmaStride; a.cap = cap; a.ld = f->ld; a.B = B;
    a.K = K; a.nSteps = nSteps; a.local = local; a.imu = f->fc.dImu; a.rec = f->fc.rec; a.out = f->fc.dOut;
    a.outStride = (long long)fc::outStride(cap); a.prm = f->prm;
    const fc::Grid gb = fc::buildGrid(B), gl = fc::lmGrid(maxN(f), B);
    hipLaunchKernelGGL(k_forecast_build, dim3(gb.x, gb.y), dim3(gb.threads), 0, f->stream, a);
    hipLaunchKernelGGL(k_forecast_lm, dim3(gl.x, gl.y), dim3(gl.threads), 0, f->stream, a);
    HIPC(hipGetLastError());
    // the filters that answer: initialised, and past their first IMU sample (a forecast does not initialise a filter)
    std::vector<int> st(B, EQF_OK);
    size_t used = 0, first = 0, end = 0;  // doubles the answering filters wrote, and the span of the image that holds them
    for (int b = 0; b < B; ++b) {
        if (!f->init[b]) st[b] = EQF_SKIPPED_NOT_INITIALISED;
        else if (f->curTime[b] < 0) st[b] = EQF_SKIPPED_BEFORE_FIRST_IMU;
        else {
            if (!used) first = fc::outStride(cap) * b;
            used += fc::outUsed(N[b]);
            end = fc::outStride(cap) * b + fc::outUsed(N[b]);
        }
    }
    // one copy for the whole batch while the span is not mostly unused capacity (a copy costs microseconds before its first byte), one per filter otherwise
    if (used && end - first <= 4 * used) {
        HIPC(hipMemcpyAsync(f->fc.hOut + first, f->fc.dOut + first, sizeof(double) * (end - first), hipMemcpyDeviceToHost, f->stream));
    } else {
        for (int b = 0; b < B; ++b)
            if (st[b] == EQF_OK)
                HIPC(hipMemcpyAsync(f->fc.hOut + fc::outStride(cap) * b, f->fc.dOut + fc::outStride(cap) * b, sizeof(double) * fc::outUsed(N[b]),
                    hipMemcpyDeviceToHost, f->stream));
    }
    HIPC(hipStreamSynchronize(f->stream));
    const double nan = std::nan("");
    for (int b = 0; b < B; ++b) {
        const double* h = f->fc.hOut + fc::outStride(cap) * b;
        const double* hb = f->fc.hOut + fc::outBase(cap, b);
        const bool skipped = st[b] != EQF_OK;
        bool numeric = false;
        if (!skipped) {
            numeric = h[fc::kHeadFlag] != 0.0;
            for (int i = 0; i < N[b] && !numeric; ++i) numeric = f->fc.hOut[fc::outLm(cap, b, i) + fc::kLmFlag] != 0.0;
            if (numeric) st[b] = EQF_ERR_NUMERIC;
            else if (nSteps > 0 && h[fc::kHeadSteps] == 0.0) st[b] = EQF_SKIPPED_NONPOSITIVE_DT;
        }
        // one value of an output: zero for a filter that was skipped, NaN for one in numeric trouble
        auto put = [&](double* dst, const double* src, int n) {
            for (int e = 0; e < n; ++e) dst[e] = skipped ? 0.0 : (numeric ? nan : src[e]);
        };
        if (out->time) put(out->time + b, h + fc::kHeadTime, 1);
        if (out->steps) out->steps[b] = (skipped || numeric) ? 0 : int(h[fc::kHeadSteps]);
        if (out->pose_q) put(out->pose_q + 4 * b, h + fc::kHeadPoseQ, 4);
        if (out->pose_x) put(out->pose_x + 3 * b, h + fc::kHeadPoseX, 3);
        if (out->velocity) put(out->velocity + 3 * b, h + fc::kHeadVel, 3);
        if (out->base) put(out->base + 121 * (size_t)b, hb, 121);
        for (int i = 0; i < (wants.perLandmark() ? stride : 0); ++i) {
            const bool live = i < N[b] && !skipped;
            static const double zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const double* l = live ? f->fc.hOut + fc::outLm(cap, b, i) : nullptr;
            const size_t row = (size_t)b * stride + i;
            // (rows behind a filter's landmarks are written as zero)
            auto putLm = [&](double* dst, int off, int n) {
                for (int e = 0; e < n; ++e) dst[e] = live ? (numeric ? nan : l[off + e]) : zeros[e];
            };
            if (out->p) putLm(out->p + 3 * row, fc::kLmP, 3);
            if (out->bearing) putLm(out->bearing + 3 * row, fc::kLmBearing, 3);
            if (out->lm) putLm(out->lm + 9 * row, fc::kLmCov, 9);
            if (out->S) putLm(out->S + 4 * row, fc::kLmS, 4);
            if (out->ycov) putLm(out->ycov + 9 * row, fc::kLmYcov, 9);
        }
        if (status) status[b] = st[b];
    }
    return EQF_OK;
}

int eqf_debug_sigma_local_all(eqf_filter* f) {
    if (!f) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    return launchLocal(f, 0, f->B, true);
}

int eqf_set_sigma(eqf_filter* f, int b, const double* src, int ld) {
    if (!f || b < 0 || b >= f->B || !src) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    const int n = kBase + 3 * int(f->ids[b].size());
    if (ld < n) return EQF_ERR_INVALID;
    f->csValid = false;  // (C Sigma / S left by an earlier burst describe the covariance that is being replaced)
    HIPC(hipStreamSynchronize(f->stream));
    for (int r = 0; r < n; ++r) std::copy(src + (size_t)r * ld, src + (size_t)r * ld + n, f->hOut + (size_t)r * n);
    HIPC(hipMemcpyAsync(f->dOut, f->hOut, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, f->stream));
    const dim3 grid((n + 256) / 256, n + 1);
    if (f->precision == EQF_PRECISION_F32)
        hipLaunchKernelGGL(k_sigma_import<float>, grid, dim3(256), 0, f->stream,
            static_cast<float*>(f->Sigma[f->pS]) + (long long)b * f->sigmaStride, f->ld, n, f->dOut, n);
    else
        hipLaunchKernelGGL(k_sigma_import<double>, grid, dim3(256), 0, f->stream,
            static_cast<double*>(f->Sigma[f->pS]) + (long long)b * f->sigmaStride, f->ld, n, f->dOut, n);
    HIPC(hipStreamSynchronize(f->stream));
    return EQF_OK;
}

int eqf_get_integrator(eqf_filter* f, int b, double* currentVelocity6, double* accumulatedVelocity6, double* accumulatedTime,
    int* initialised) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    GATE(f);
    Glob g;
    int rc = fetchGlob(f, b, &g);
    if (rc) return rc;
    if (currentVelocity6) std::copy(g.curVel, g.curVel + 6, currentVelocity6);
    if (accumulatedVelocity6) std::copy(g.accVel, g.accVel + 6, accumulatedVelocity6);
    if (accumulatedTime) *accumulatedTime = g.accTime;
    if (initialised) *initialised = g.initialised;
    return EQF_OK;
}

int eqf_set_state(eqf_filter* f, int b, int N, const int* ids, const double* pose_q, const double* pose_x, const double* velocity,
    const double* p0, const double* A_q, const double* A_x, const double* w, const double* Q_q, const double* Q_a, const double* bias6,
    const double* sigma, int ld, double currentTime, const double* currentVelocity6, const double* accumulatedVelocity6,
    double accumulatedTime, int initialised) {
    if (!f || b < 0 || b >= f->B || N < 0 || !pose_q || !pose_x || !velocity || !A_q || !A_x || !w || !bias6 || !sigma) return EQF_ERR_INVALID;
    GATE(f);
    if (N > 0 && (!ids || !p0 || !Q_q || !Q_a)) return EQF_ERR_INVALID;
    if (N > f->cap) return EQF_ERR_CAPACITY;
    if (ld < kBase + 3 * N) return EQF_ERR_INVALID;
    HIPC(hipSetDevice(f->device));
    Glob g;
    int rc = fetchGlob(f, b, &g);
    if (rc) return rc;
    std::copy(pose_q, pose_q + 4, g.P0q);
    std::copy(pose_x, pose_x + 3, g.P0x);
    std::copy(velocity, velocity + 3, g.v0);
    std::copy(A_q, A_q + 4, g.Aq);
    std::copy(A_x, A_x + 3, g.Ax);
    std::copy(w, w + 3, g.w);
    std::copy(bias6, bias6 + 6, g.bias);
    for (int i = 0; i < 6; ++i) {
        g.curVel[i] = currentVelocity6 ? currentVelocity6[i] : 0.0;
        g.accVel[i] = accumulatedVelocity6 ? accumulatedVelocity6[i] : 0.0;
    }
    g.accTime = accumulatedTime;
    g.curTime = currentTime;
    g.initialised = initialised ? 1 : 0;
    g.N = N;
    g.updateOk = 0;
    HIPC(hipMemcpy(f->g[f->pG] + b, &g, sizeof(Glob), hipMemcpyHostToDevice));
    const int cap = f->cap;
    std::vector<double> tp((size_t)3 * cap, 0.0), tq((size_t)5 * cap, 0.0);
    for (int i = 0; i < N; ++i) {
        for (int c = 0; c < 3; ++c) tp[(size_t)c * cap + i] = p0[3 * i + c];
        for (int c = 0; c < 4; ++c) tq[(size_t)c * cap + i] = Q_q[4 * i + c];
        tq[(size_t)4 * cap + i] = Q_a[i];
    }
    HIPC(hipMemcpy(f->p0 + (size_t)b * 3 * cap, tp.data(), sizeof(double) * 3 * cap, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(f->Q[f->pG] + (size_t)b * 5 * cap, tq.data(), sizeof(double) * 5 * cap, hipMemcpyHostToDevice));
    f->ids[b].assign(ids, ids + N);
    f->report[b] = {};
    f->curTime[b] = currentTime;
    f->init[b] = initialised ? 1 : 0;
    f->devInit[b] = f->init[b];
    hipLaunchKernelGGL(k_restore_constants, dim3((N + 127) / 128 + 1), dim3(128), 0, f->stream, f->g[f->pG], b, f->p0, f->lmc, cap, f->errflag);
    HIPC(hipGetLastError());
    rc = eqf_set_sigma(f, b, sigma, ld);  // (synchronises)
    if (rc) return rc;
    // Recovery from a hand-off time-out (bit 128 of the sticky flag, include/eqf_vio_amd.h): the launch that timed out wrote no covariance,
    // and once EVERY filter of the handle has been given a state again nothing of it is left -- the bit is cleared (the other bits are
    // the caller's to look at: eqf_reset clears those) and k_edit's barrier counters, which a timed-out launch leaves mid-count, start
    // from zero.  With batch = 1 that is this very call.
    if (f->restoredMark.size() != (size_t)f->B) f->restoredMark.assign(f->B, 0);
    int e = 0;
    HIPC(hipMemcpy(&e, f->errflag, sizeof(int), hipMemcpyDeviceToHost));
    if (!(e & 128)) {
        f->restoredMark.assign(f->B, 0);  // (no time-out to recover from: restores of a healthy handle are not counted towards a later one)
    } else {
        f->restoredMark[b] = 1;
    }
    if ((e & 128) && std::all_of(f->restoredMark.begin(), f->restoredMark.end(), [](char c) { return c != 0; })) {
        f->restoredMark.assign(f->B, 0);
        {
            // (bit 4 with it: a chain that unwinds may have judged a pivot of operands it never received -- a by-product of the time-out)
            e &= ~(128 | 4);
            HIPC(hipMemcpy(f->errflag, &e, sizeof(int), hipMemcpyHostToDevice));
            if (f->dEditBar) HIPC(hipMemset(f->dEditBar, 0, sizeof(int) * 4 * f->B));
        }
    }
    return EQF_OK;
}

// The small state of a handle as eqf_clone.hpp's kernels see it (current parity of Glob and Q).
static CloneSide cloneSide(eqf_filter* f) {
    CloneSide s{};
    s.g = f->g[f->pG]; s.p0 = f->p0; s.Q = f->Q[f->pG];
    s.delta = f->dbgDelta; s.gamma = f->dbgGamma; s.gammaTot = f->dbgGammaTot;
    s.innov = (f->innovStats && f->dInnov) ? f->dInnov : nullptr;
    s.cap = f->cap;
    return s;
}
// ... and of the staging image of the in-place case: one allocation in the handle's own layout (clone::SmallLayout)
static_assert(clone::kPadBase == kLm0 && clone::kOk == EQF_OK && clone::kInvalid == EQF_ERR_INVALID && clone::kCapacity == EQF_ERR_CAPACITY &&
                  sizeof(clone::Pair) == sizeof(ClonePair) && offsetof(clone::Pair, dst) == offsetof(ClonePair, dst) &&
                  offsetof(clone::Pair, src) == offsetof(ClonePair, src) && offsetof(clone::Pair, N) == offsetof(ClonePair, N) &&
                  offsetof(clone::Pair, fromStage) == offsetof(ClonePair, fromStage) && sizeof(Glob) % sizeof(double) == 0,
    "eqf_clone_host.hpp repeats the layout constants, the pair table and the error codes");
static CloneSide cloneStageSide(eqf_filter* f) {
    const clone::SmallLayout sl = cloneSmall(f);
    char* p = f->clone.small;
    auto doubles = [p](size_t off) { return reinterpret_cast<double*>(p + off); };
    CloneSide s{};
    s.g = reinterpret_cast<Glob*>(p + sl.offGlob());
    s.p0 = doubles(sl.offP0()); s.Q = doubles(sl.offQ()); s.delta = doubles(sl.offDelta()); s.gamma = doubles(sl.offGamma());
    s.gammaTot = doubles(sl.offGammaTot());
    s.innov = (f->innovStats && f->dInnov) ? doubles(sl.offInnov()) : nullptr;
    s.cap = f->cap;
    return s;
}
// the launches of a pair table (nPairs > 0) on `st`: covariance and small state; into a handle (ma.restore) also what k_restore_constants does
static void launchClone(eqf_filter* dst, hipStream_t st, const CloneSigmaArgs& sa, const CloneSmallArgs& ma, int nMaxN) {
    const int n = kLm0 + 3 * nMaxN, kV = dst->precision == EQF_PRECISION_F32 ? 4 : 2;
    const dim3 grid((n + 256 * kV - 1) / (256 * kV), (n + kCloneRows - 1) / kCloneRows, std::min(sa.nPairs, 65535));
    if (dst->precision == EQF_PRECISION_F32) hipLaunchKernelGGL(k_clone_sigma<float>, grid, dim3(256), 0, st, sa);
    else hipLaunchKernelGGL(k_clone_sigma<double>, grid, dim3(256), 0, st, sa);
    const int np = std::min(ma.nPairs, 65535);
    hipLaunchKernelGGL(k_clone_small, dim3(std::max(1, (dst->cap + 255) / 256), np), dim3(256), 0, st, ma);
    if (ma.restore)
        hipLaunchKernelGGL(k_clone_restore, dim3(std::max(1, (nMaxN + 127) / 128), np), dim3(128), 0, st, dst->g[dst->pG], dst->p0, dst->lmc, dst->cap,
            dst->errflag, ma.pairs, ma.nPairs);
}

int eqf_copy_filters(eqf_filter* dst, eqf_filter* src, int n, const int* dst_idx, const int* src_idx) {
    if (!dst || !src || !dst_idx || !src_idx || n < 0) return EQF_ERR_INVALID;
    int rc = clone::headCheck(dst->B, src->B, n, dst_idx, src_idx);
    if (rc) return rc;
    if (dst->precision != src->precision || dst->device != src->device) return EQF_ERR_UNSUPPORTED;
    if (n == 0) return EQF_OK;
    GATE(dst);
    if (src != dst) GATE(src);
    const bool inPlace = dst == src;
    // the pairs that move something, and those that bring a source to the staging image first (the landmark counts are settled now)
    std::vector<clone::Pair> pairs, stagePairs;
    int nMaxN = 0;
    rc = clone::plan(dst->B, src->B, dst->cap, inPlace, n, dst_idx, src_idx, landmarkCounts(src).data(), pairs, stagePairs, nMaxN);
    if (rc) return rc;
    if (pairs.empty()) return EQF_OK;
    // everything that can fail is had before anything is written
    const int nTab = int(pairs.size() + stagePairs.size());
    {
        const bool stages = !stagePairs.empty();
        const workspace::Want wd[] = {want(dst->clone.evDone), want(dst->clone.hPairs, sizeof(ClonePair) * nTab, &dst->clone.pairsCap),
            want(dst->clone.dPairs, sizeof(ClonePair) * nTab, &dst->clone.pairsCap), sigmaLocWant(dst, stages),
            want(dst->clone.small, stages ? cloneSmall(dst).bytes() : 0)};
        const workspace::Want ws[] = {want(src->clone.evSrc)};
        rc = reserveSlots(dst, wd);
        if (!rc) rc = reserveSlots(src, ws);
        if (rc) return rc;
    }
    HIPC(hipEventSynchronize(dst->clone.evDone));  // (the previous copy into this handle has read its pair table)
    hipStream_t st = dst->stream;
    if (!inPlace) {  // the copy sees what the source has enqueued
        HIPC(hipEventRecord(src->clone.evSrc, src->stream));
        HIPC(hipStreamWaitEvent(st, src->clone.evSrc, 0));
    }
    std::memcpy(dst->clone.hPairs.get(), pairs.data(), sizeof(ClonePair) * pairs.size());
    if (!stagePairs.empty()) std::memcpy(dst->clone.hPairs + pairs.size(), stagePairs.data(), sizeof(ClonePair) * stagePairs.size());
    HIPC(hipMemcpyAsync(dst->clone.dPairs, dst->clone.hPairs, sizeof(ClonePair) * nTab, hipMemcpyHostToDevice, st));
    CloneSigmaArgs sa{};
    sa.src = src->Sigma[src->pS]; sa.stage = dst->dSigmaLoc; sa.dst = dst->Sigma[dst->pS];
    sa.ldSrc = src->ld; sa.ldDst = dst->ld; sa.strideSrc = src->sigmaStride; sa.strideDst = dst->sigmaStride;
    sa.pairs = dst->clone.dPairs; sa.nPairs = int(pairs.size());
    CloneSmallArgs ma{};
    ma.src = cloneSide(src); ma.dst = cloneSide(dst); ma.restore = 1;
    ma.pairs = dst->clone.dPairs; ma.nPairs = int(pairs.size());
    if (!stagePairs.empty()) {
        int nStageN = 0;
        for (auto& p : stagePairs) nStageN = std::max(nStageN, p.N);
        CloneSigmaArgs ss = sa;
        ss.dst = dst->dSigmaLoc;
        ss.pairs = dst->clone.dPairs + pairs.size(); ss.nPairs = int(stagePairs.size());
        CloneSmallArgs ms = ma;
        ms.dst = cloneStageSide(dst); ms.restore = 0;
        ms.pairs = ss.pairs; ms.nPairs = ss.nPairs;
        ma.stage = ms.dst;
        launchClone(dst, st, ss, ms, nStageN);
    }
    launchClone(dst, st, sa, ma, nMaxN);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(dst->clone.evDone, st));
    if (!inPlace) HIPC(hipStreamWaitEvent(src->stream, dst->clone.evDone, 0));  // (the source's later work flips its buffers: not before the copy has read them)
    // host mirrors (read first: in place a destination may be a source); the caches that describe the device's landmark sets start over
    std::vector<Mirror> mirrors;
    mirrors.reserve(pairs.size());
    for (const auto& p : pairs) mirrors.push_back(mirrorOf(src, p.src));
    for (size_t k = 0; k < pairs.size(); ++k) adoptMirror(dst, pairs[k].dst, std::move(mirrors[k]));
    forgetDeviceCaches(dst);
    return EQF_OK;
}

// ---- explicit landmark removal and insertion with priors (eqf_mapedit.hpp; the host's decisions: eqf_mapedit_host.hpp)
static_assert(mapedit::kPrior == kMapPrior && mapedit::kOk == EQF_OK && mapedit::kInvalid == EQF_ERR_INVALID &&
                  mapedit::kCapacity == EQF_ERR_CAPACITY && mapedit::kUnsorted == EQF_ERR_UNSORTED,
    "eqf_mapedit_host.hpp repeats the layout constants and the error codes");
namespace {
// the plan's image, from capacity and batch
int mapEditReserve(eqf_filter* f) {
    const workspace::Want w[] = {WANT_STAGED(f->medit.img, mapedit::imageCapacityBytes(f->B, f->cap))};
    return reserveSlots(f, w);
}
}  // namespace

int eqf_edit_landmarks(eqf_filter* f, const int* n_remove, const int* remove_ids, int rstride, const int* n_insert, const int* insert_ids,
    int istride, const double* p, const double* P, unsigned char* removed, unsigned char* inserted) {
    if (!f) return EQF_ERR_INVALID;
    GATE(f);  // (queued IMU calls and a pending gate first: the gate may still change the landmark lists)
    const int B = f->B, cap = f->cap;
    const mapedit::Args ma{n_remove, remove_ids, rstride, n_insert, insert_ids, istride, p, P};
    mapedit::Plan pl;
    int rc = mapedit::plan(f->ids, cap, ma, pl);
    if (rc) return rc;
    const bool work = pl.anyRemoved || pl.anyInserted;
    if (work) {
        rc = mapEditReserve(f);
        if (rc) return rc;
    }
    if (removed) std::copy(pl.removed.begin(), pl.removed.end(), removed);
    if (inserted) std::copy(pl.inserted.begin(), pl.inserted.end(), inserted);
    if (!work) return EQF_OK;
    const mapedit::Image im = mapedit::imageLayout(B, cap, pl);
    HIPC(f->medit.img.wait());
    mapedit::fillImage(f->ids, ma, pl, im, f->medit.img.host);
    HIPC(f->medit.img.upload(im.bytes(), f->stream));
    MapEditArgs a{};
    a.g = f->g[f->pG];
    a.prior = reinterpret_cast<const double*>(f->medit.img.dev + im.offPrior());
    a.cnt = reinterpret_cast<const int*>(f->medit.img.dev + im.offCounts());
    a.map = reinterpret_cast<const int*>(f->medit.img.dev + im.offMap());
    a.ns = int(im.ns); a.cap = cap;
    a.p0 = f->p0; a.Q = f->Q[f->pG]; a.lmc = f->lmc; a.scratch = f->dScratch; a.errflag = f->errflag;
    a.sigmaStride = f->sigmaStride; a.ld = f->ld;
    if (pl.anyRemoved) {
        a.Sin = f->Sigma[f->pS]; a.Sout = f->Sigma[f->pS ^ 1];
        const int nvn = kLm0 + 3 * pl.maxN;
        const dim3 grid((nvn + 255) / 256, (nvn + 3) / 4, B);
        rc = profiled(f, EQF_PROF_CHURN, [&] {
            withSigmaType(f, [&](auto t) { hipLaunchKernelGGL(k_mapedit_move<decltype(t)>, grid, dim3(256), 0, f->stream, a); });
        });
    } else {
        a.Sin = nullptr; a.Sout = f->Sigma[f->pS];
        const long long work1 = (long long)3 * pl.maxNew * (kLm0 + 3 * pl.maxN) * 2;
        const dim3 grid(int(std::max<long long>(1, std::min<long long>(1024, (work1 + 255) / 256))), B);
        rc = profiled(f, EQF_PROF_CHURN, [&] {
            withSigmaType(f, [&](auto t) { hipLaunchKernelGGL(k_mapedit_append<decltype(t)>, grid, dim3(256), 0, f->stream, a); });
        });
    }
    if (rc) return rc;
    HIPC(hipGetLastError());
    if (pl.anyRemoved) f->pS ^= 1;
    f->ids = std::move(pl.newIds);
    forgetDeviceCaches(f);
    return EQF_OK;
}

int eqf_set_camera_offset(eqf_filter* f, const double* q, const double* x) {
    if (!f || !q || !x) return EQF_ERR_INVALID;
    GATE(f);
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(std::fabs(n2 - 1.0) < 1e-6)) return EQF_ERR_INVALID;
    HIPC(hipSetDevice(f->device));
    HIPC(hipStreamSynchronize(f->stream));
    std::copy(q, q + 4, f->prm.camq);
    std::copy(x, x + 3, f->prm.camx);
    std::copy(q, q + 4, f->set.cameraOffset_q);
    std::copy(x, x + 3, f->set.cameraOffset_x);
    setCameraConstants(f->prm);
    return EQF_OK;
}

int eqf_get_last_update(eqf_filter* f, int b, double* delta, double* gamma, double* Gamma) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    HIPC(hipStreamSynchronize(f->stream));
    const int N = int(f->ids[b].size()), cap = f->cap;
    if (delta) HIPC(hipMemcpy(delta, f->dbgDelta + (size_t)b * 2 * cap, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
    if (gamma) {
        std::vector<double> tmp(kLm0 + 3 * N);
        HIPC(hipMemcpy(tmp.data(), f->dbgGamma + (size_t)b * (kLm0 + 3 * cap), sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < kBase; ++i) gamma[i] = tmp[i];
        for (int i = 0; i < 3 * N; ++i) gamma[kBase + i] = tmp[kLm0 + i];
    }
    if (Gamma) HIPC(hipMemcpy(Gamma, f->dbgGammaTot + (size_t)b * (9 + 3 * cap), sizeof(double) * (9 + 3 * N), hipMemcpyDeviceToHost));
    return EQF_OK;
}

int eqf_debug_launch_shape(eqf_filter* f, int* shape8) {
    if (!f || !shape8) return EQF_ERR_INVALID;
    std::copy(f->lastBurstShape, f->lastBurstShape + 8, shape8);
    return EQF_OK;
}

int eqf_debug_get_blocks(eqf_filter* f, int b, double* common, double* rec, double* c0) {
    if (!f || b < 0 || b >= f->B) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    HIPC(hipStreamSynchronize(f->stream));
    const int N = int(f->ids[b].size()), cap = f->cap;
    if (common) {
        CommonLds c;
        HIPC(hipMemcpy(&c, f->dBlkCommon + b, sizeof(CommonLds), hipMemcpyDeviceToHost));
        common[0] = c.T;
        std::copy(c.Bg, c.Bg + 6, common + 1);
        std::copy(c.Bvw, c.Bvw + 9, common + 7);
        std::copy(c.RA, c.RA + 9, common + 16);
        std::copy(c.Avg, c.Avg + 6, common + 25);
    }
    if (rec && N > 0) {
        std::vector<double> tmp((size_t)kBlkRec * N);
        HIPC(hipMemcpy(tmp.data(), static_cast<const double*>(f->dBlk) + (size_t)b * cap * kBlkRec, sizeof(double) * tmp.size(),
            hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i) std::copy(&tmp[(size_t)i * kBlkRec], &tmp[(size_t)i * kBlkRec] + 27, rec + (size_t)27 * i);
    }
    if (c0 && N > 0) {
        std::vector<double> tmp((size_t)15 * cap);
        HIPC(hipMemcpy(tmp.data(), f->lmc + (size_t)b * 15 * cap, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < N; ++i)
            for (int q = 0; q < 6; ++q) c0[(size_t)6 * i + q] = tmp[(size_t)q * cap + i];
    }
    return EQF_OK;
}

int eqf_device_error(eqf_filter* f) {
    if (!f) return EQF_ERR_INVALID;
    if (resolveGate(f) || flushBurst(f)) return EQF_ERR_HIP;
    if (hipSetDevice(f->device) != hipSuccess) return EQF_ERR_HIP;
    if (hipStreamSynchronize(f->stream) != hipSuccess) return EQF_ERR_HIP;
    int e = 0;
    if (hipMemcpy(&e, f->errflag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return EQF_ERR_HIP;
    return e;
}

int eqf_debug_drop_role(eqf_filter* f, int kind, int role, int R, int C) {
    if (!f || kind > 1 || (kind >= 0 && (role < 0 || role > 2))) return EQF_ERR_INVALID;
    GATE(f);
    f->dropRole[0] = kind; f->dropRole[1] = role; f->dropRole[2] = R; f->dropRole[3] = C;
    f->rolesN = -1;  // the role table is rebuilt by the next update
    return EQF_OK;
}

int eqf_debug_option(eqf_filter* f, const char* name, int value) {
    if (!f || !name) return EQF_ERR_INVALID;
    GATE(f);
    if (!std::strcmp(name, "e_sigma_min_percu_x10")) {
        f->eSigmaMinPerCU = value / 10.0;
        return EQF_OK;
    }
    if (!std::strcmp(name, "burst_fused_max_x10")) {
        f->fusedMaxPerCU = value / 10.0;
        return EQF_OK;
    }
    if (!std::strcmp(name, "ring_ahead2")) {
        f->ringAhead2 = value ? 1 : 0;
        return EQF_OK;
    }
    if (!std::strcmp(name, "burst_lm")) {  // landmarks per builder workgroup: 0 = by launch size, 4 / 8 / 16
        if (value != 0 && value != 4 && value != 8 && value != 16) return EQF_ERR_INVALID;
        f->burstLm = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "burst_rows")) {  // row landmarks per wavefront of the block kernel: 0 = by launch size, 1 / 2 / 4
        if (value != 0 && value != 1 && value != 2 && value != 4) return EQF_ERR_INVALID;
        f->burstRows = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "res_tickets")) {
        if (value < 0 || value > 2) return EQF_ERR_INVALID;
        f->resTickets = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "res_border")) {
        if (value != 0 && value != 1) return EQF_ERR_INVALID;
        f->resBorder = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "device_edit")) {
        f->deviceEdit = value ? 1 : 0;
        return EQF_OK;
    }
    if (!std::strcmp(name, "cs_in_burst")) {
        f->csInBurst = value;
        f->csValid = false;
        return EQF_OK;
    }
    return EQF_ERR_INVALID;
}

int eqf_set_option(eqf_filter* f, const char* name, int value) {
    if (!f || !name) return EQF_ERR_INVALID;
    if (!std::strcmp(name, "downdate_slices")) {
        if (value != 0 && (value < 5 || value > 7)) return EQF_ERR_INVALID;
        if (value && f->precision == EQF_PRECISION_F32) return EQF_ERR_UNSUPPORTED;
        GATE(f);
        if (value > f->i8Slices) {
            // workspace from the capacity: the slices of every filter's Y (mp x nv at most) and one exponent word per column
            const int nvCap = kLm0 + 3 * f->cap, mpCap = roundUp(sDim(f->cap), kSB);
            if (!i8Exact(mpCap, value)) return EQF_ERR_CAPACITY;  // (int32 accumulation would no longer be exact: capacity > ~37 000)
            const long long stride = i8SliceBytes(mpCap, nvCap, value);
            const workspace::Want w[] = {want(f->dI8Ws, size_t(stride) * f->B, &f->i8WsBytes),
                want(f->dI8Expo, sizeof(int) * size_t(i8ddExpoWords(nvCap)) * f->B)};
            const int rc = reserveSlots(f, w);
            if (rc) return rc;
            f->i8WsStride = stride;
            f->i8Slices = value;
        }
        f->ddSlices = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "res_tickets")) {
        if (value < 0 || value > 2) return EQF_ERR_INVALID;
        GATE(f);
        f->resTickets = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "innovation_stats")) {
        if (value != 0 && value != 1) return EQF_ERR_INVALID;
        if (value && f->precision == EQF_PRECISION_F32) return EQF_ERR_UNSUPPORTED;
        GATE(f);
        if (value && !f->dInnov) {
            const workspace::Want w[] = {want(f->dInnov, sizeof(double) * cloneSmall(f).innovCount() * f->B)};
            const int rc = reserveSlots(f, w);
            if (rc) return rc;
        }
        // (switching the option, either way, forgets the last update's statistics)
        if (f->dInnov) HIPC(hipMemsetAsync(f->dInnov, 0, sizeof(double) * (size_t)(kInnovHead + f->cap) * f->B, f->stream));
        f->innovStats = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "innovation_lift")) {  // eqf_lift.hpp: 0 the plain lift, 1 the handle's useInnovationLift / useDiscreteInnovationLift
        if (!lift::optionOk(value)) return EQF_ERR_INVALID;
        if (f->precision == EQF_PRECISION_F32) return EQF_ERR_UNSUPPORTED;
        f->lift.opt = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "merge_cost_chunk")) {  // images per round of eqf_get_merge_costs (0: as many as the handle has filters)
        if (value != 0 && !mergecost::chunkOptionOk(value)) return EQF_ERR_INVALID;
        f->mc.chunkOpt = value;
        return EQF_OK;
    }
    if (!std::strcmp(name, "score_chunk")) {  // images per round of eqf_score_vision (0: as many as the handle has filters)
        if (value != 0 && !score::chunkOptionOk(value)) return EQF_ERR_INVALID;
        f->sc.chunkOpt = value;
        return EQF_OK;
    }
    return EQF_ERR_INVALID;
}

int eqf_set_outlier_gate(eqf_filter* f, int kind, double threshold) {
    if (!f || (kind != EQF_GATE_CHORD && kind != EQF_GATE_MAHALANOBIS) || threshold != threshold) return EQF_ERR_INVALID;
    if (kind == EQF_GATE_MAHALANOBIS && !(threshold > 0.0)) return EQF_ERR_INVALID;
    if (kind == EQF_GATE_MAHALANOBIS && f->precision == EQF_PRECISION_F32) return EQF_ERR_UNSUPPORTED;
    GATE(f);  // (a pending speculative gate is resolved with the kind and the threshold it was evaluated under)
    f->gateKind = kind;
    f->gateThr = threshold;
    return EQF_OK;
}

int eqf_get_outlier_gate(eqf_filter* f, int* kind, double* threshold) {
    if (!f) return EQF_ERR_INVALID;
    if (kind) *kind = f->gateKind;
    if (threshold) *threshold = f->gateThr;
    return EQF_OK;
}

int eqf_get_gate_report(eqf_filter* f, int b, int* n, int* ids, double* stat, int* removed) {
    if (!f || b < 0 || b >= f->B || !n) return EQF_ERR_INVALID;
    GATE(f);
    const auto& r = f->report[b];
    *n = int(r.ids.size());
    if (ids) std::copy(r.ids.begin(), r.ids.end(), ids);
    if (stat) std::copy(r.stat.begin(), r.stat.end(), stat);
    if (removed) std::copy(r.removed.begin(), r.removed.end(), removed);
    return EQF_OK;
}

int eqf_get_innovation_stats(eqf_filter* f, int b, eqf_innovation_stats* out, double* nis_lm) {
    if (!f || b < 0 || b >= f->B || !out) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    HIPC(hipStreamSynchronize(f->stream));
    std::memset(out, 0, sizeof(*out));
    if (!f->innovStats || !f->dInnov) return EQF_OK;
    const int N = int(f->ids[b].size());
    std::vector<double> tmp(kInnovHead + (size_t)N);
    HIPC(hipMemcpy(tmp.data(), f->dInnov + (size_t)b * (kInnovHead + f->cap), sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    if (tmp[4] == 0.0) return EQF_OK;
    out->nis = tmp[0];
    out->logdet_S = tmp[1];
    out->loglik = tmp[3];
    out->dof = int(tmp[2]);
    out->valid = 1;
    if (nis_lm) std::copy(tmp.begin() + kInnovHead, tmp.end(), nis_lm);
    return EQF_OK;
}

// the buffers of eqf_get_nees and of the draws' factorisation, from capacity and batch
static_assert(sample::kRecHead == kNeesHead && sample::kTileRows == kNeesRhs, "eqf_sample_host.hpp repeats the layout constants");
static int neesReserve(eqf_filter* f) {
    const size_t B = size_t(f->B);
    const workspace::Want w[] = {want(f->nees.E, sizeof(double) * size_t(kNeesRhs) * f->ld * B), want(f->nees.D, sizeof(double) * size_t(kDRec) * B),
        want(f->nees.out, sample::RecordsLayout{B}.bytes()), want(f->nees.bad, sizeof(int) * B), sigmaLocWant(f)};
    return reserveSlots(f, w);
}

// A = L L^T of every filter's submatrix from internal index off, in place in the scratch image -- Sigma_loc (k_sigma_local) or a copy of
// Sigma --, the nrhs error vectors that lie in nees.E carried along, and k_nees_tail's report in nees.out: what eqf_get_nees and the draws
// (nrhs = 0) share.  Enqueues; the buffers are there (neesReserve).
static int neesFactor(eqf_filter* f, int local, int off, int nrhs) {
    const int B = f->B, mMax = kLm0 + 3 * maxN(f) - off;
    int rc = EQF_OK;
    if (local) {
        rc = launchLocal(f, 0, B, true);
        if (rc) return rc;
    } else {
        HIPC(hipMemcpyAsync(f->dSigmaLoc, f->Sigma[f->pS], sizeof(double) * size_t(f->sigmaStride) * B, hipMemcpyDeviceToDevice, f->stream));
    }
    NeesArgs a{};
    a.g = f->g[f->pG]; a.A = f->dSigmaLoc; a.ld = f->ld; a.strideA = f->sigmaStride; a.E = f->nees.E; a.ldE = std::max(mMax, 1); a.D = f->nees.D;
    a.bad = f->nees.bad; a.jac = local ? f->dJac : nullptr; a.cap = f->cap; a.off = off; a.nrhs = nrhs; a.out = f->nees.out;
    rc = enqueueFactor(f->stream, f->nees.ldsSet, a, B, mMax, nrhs > 0 ? 1 : 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nees_tail, dim3(B), dim3(256), 0, f->stream, a);
    HIPC(hipGetLastError());
    return EQF_OK;
}
// k_nees_tail's records (sample::RecordsLayout) brought to the host; returns once they are there
static int readNeesRecords(eqf_filter* f, std::vector<double>& hO) {
    hO.resize(sample::RecordsLayout{size_t(f->B)}.doubles());
    HIPC(hipMemcpyAsync(hO.data(), f->nees.out, sizeof(double) * hO.size(), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    return EQF_OK;
}
// ... -> the caller's
static void neesStats(const double* hO, int B, eqf_sigma_stats* stats) {
    const sample::RecordsLayout rl{size_t(B)};
    for (int b = 0; b < B; ++b) {
        const double* o = hO + rl.offRecord(b);
        stats[b].logdet = o[0];
        stats[b].min_pivot = o[1];
        stats[b].dof = int(o[2]);
        stats[b].info = int(o[3]);
    }
}

int eqf_get_nees(eqf_filter* f, int local, int first, int nrhs, const double* err, int lde, double* nees, eqf_sigma_stats* stats) {
    if (!f || !stats || (local != 0 && local != 1) || (first != 0 && first != 6 && first != kBase) || nrhs < 0 || nrhs > kNeesRhs)
        return EQF_ERR_INVALID;
    if (nrhs > 0 && (!err || !nees)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);  // (a pending outlier gate may still change the landmark counts: settle them before they are looked at)
    const int B = f->B, nMax = maxN(f);
    if (nrhs > 0 && lde < kBase + 3 * nMax) return EQF_ERR_INVALID;
    int rc = neesReserve(f);
    if (rc) return rc;
    const int off = first == kBase ? kLm0 : first, ldE = std::max(kLm0 + 3 * nMax - off, 1);
    // the error vectors in the submatrix' own (padded) index map: entry i of the reference -> column (i < 11 ? i : i + 1) - off
    std::vector<double> hE;
    if (nrhs > 0) {
        hE.assign(size_t(B) * nrhs * ldE, 0.0);
        for (int b = 0; b < B; ++b) {
            const int n = kBase + 3 * int(f->ids[b].size());
            for (int k = 0; k < nrhs; ++k) {
                const double* src = err + (size_t(b) * nrhs + k) * lde;
                double* dst = hE.data() + (size_t(b) * nrhs + k) * ldE;
                for (int i = first; i < n; ++i) dst[(i < kBase ? i : i + 1) - off] = src[i];
            }
        }
        HIPC(hipMemcpyAsync(f->nees.E, hE.data(), sizeof(double) * hE.size(), hipMemcpyHostToDevice, f->stream));
    }
    rc = neesFactor(f, local, off, nrhs);
    if (rc) return rc;
    std::vector<double> hO;
    rc = readNeesRecords(f, hO);
    if (rc) return rc;
    neesStats(hO.data(), B, stats);
    const sample::RecordsLayout rl{size_t(B)};
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nrhs; ++k) nees[size_t(b) * nrhs + k] = hO[rl.offNees(b, k)];
    return EQF_OK;
}

// ---- the innovation lift of the calls that inform a filter outside a vision frame (eqf_lift.hpp; decisions and layout: eqf_lift_host.hpp)
static_assert(lift::kRefBase == kBase && lift::kPadBase == kLm0 && lift::kOff == kLiftOff && lift::kRhs == kLiftRhs && lift::kRec == kLiftRec &&
              lift::kHead == kLiftHead && kLiftHead == kLinHead && lift::kWordFailed == kLiftWordFailed &&
              lift::kWordFailed != blocks::kInfoIdle && lift::kWordIdle == blocks::kInfoIdle && lift::kPadPos == kBase - kLiftOff,
    "eqf_lift_host.hpp repeats the layout constants");
static_assert(border::kBlock == kSB && border::kStage == kQB && border::kRows == kBorderRows, "eqf_border_host.hpp repeats the layout constants");
namespace {
int liftCallKind(const eqf_filter* f) { return lift::callKind(f->lift.opt, f->prm.useInnovationLift, f->prm.useDiscreteInnovationLift); }
// lift::updateReport's fields as the C ABI has them
eqf_linear_report linearReport(const lift::UpdateReport& r) { return eqf_linear_report{r.nis, r.logdet_S, r.loglik, r.dof, r.info}; }
// What a call needs before any effect: the records always, the factorisation's buffers where the call factors.
int liftReserve(eqf_filter* f, bool factors) {
    const size_t B = size_t(f->B);
    const workspace::Want w[] = {want(f->lift.rec, sizeof(double) * size_t(kLiftRec) * B),
        want(f->lift.E, factors ? sizeof(double) * lift::rhsDoubles(f->ld) * B : 0), want(f->lift.D, factors ? sizeof(double) * size_t(kDRec) * B : 0),
        want(f->lift.bad, factors ? sizeof(int) * B : 0), sigmaLocWant(f, factors)};
    return reserveSlots(f, w);
}
// Enqueues the lift of a call behind the launches that left its increment (filter b: gamma[b * strideG + j], internal index offG + j) and,
// for an update, its verdict (records [B][kLinHead], entry 3) -- and in front of whatever changes Sigma: a device copy of Sigma, the
// right-hand side, the factorisation and the tail where some filter takes a bundleLift, the tail alone (the records) otherwise.  The
// filters the tail has not dealt with are k_apply_increment's: its IncArgs get the records.  (liftReserve has run.)
int liftEnqueue(eqf_filter* f, const double* gamma, long long strideG, int offG, const unsigned char* dMask, double* verdict, bool writesVerdict,
    IncArgs& ia) {
    const int B = f->B, nMax = maxN(f), kind = liftCallKind(f);
    LiftArgs a{};
    a.g = f->g[f->pG]; a.p0 = f->p0; a.Q = f->Q[f->pG]; a.cap = f->cap; a.A = f->dSigmaLoc; a.ld = f->ld; a.strideA = f->sigmaStride;
    a.E = f->lift.E; a.ldE = lift::rhsPitch(nMax); a.D = f->lift.D; a.bad = f->lift.bad; a.gamma = gamma; a.strideG = strideG; a.offG = offG;
    a.mask = dMask; a.verdict = verdict; a.fail = writesVerdict ? verdict : nullptr; a.kind = lift::callFactors(kind, nMax) ? kind : 0;
    a.rec = f->lift.rec; a.prm = f->prm;
    if (a.kind) {
        HIPC(hipMemcpyAsync(f->dSigmaLoc, f->Sigma[f->pS], sizeof(double) * size_t(f->sigmaStride) * B, hipMemcpyDeviceToDevice, f->stream));
        hipLaunchKernelGGL(k_lift_rhs, dim3(lift::rhsGroups(nMax), B), dim3(256), 0, f->stream, a);
        const int rc = enqueueFactor(f->stream, f->lift.ldsSet, a, B, lift::order(nMax), 1);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_lift_tail, dim3(B), dim3(256), 0, f->stream, a);
    HIPC(hipGetLastError());
    f->lift.called = true;
    ia.lift = f->lift.rec;
    ia.liftStride = kLiftRec;
    return EQF_OK;
}

// ---- the Schmidt (consider) variants (eqf_schmidt.hpp; the host's decisions: eqf_schmidt_host.hpp)
static_assert(schmidt::kOk == EQF_OK && schmidt::kInvalid == EQF_ERR_INVALID && schmidt::kCapacity == EQF_ERR_CAPACITY &&
                  schmidt::kUnsorted == EQF_ERR_UNSORTED && schmidt::kPadBase == kLm0 && schmidt::kTile == kSB,
    "eqf_schmidt_host.hpp repeats the layout constants and the error codes");
// the consider lists of a call as the C ABI has them
struct SchCall {
    const int* n;
    const int* ids;
    int cstride;
};
// the partition's image, from capacity and batch
int schReserve(eqf_filter* f) {
    const workspace::Want w[] = {WANT_STAGED(f->sch.img, (schmidt::Image{size_t(f->B), size_t(f->ld)}.bytes()))};
    return reserveSlots(f, w);
}
// Builds every filter's partition from the handle's id mirror in the pinned image (schReserve has run, the lists are checked); the launch of
// k_schmidt_gamma brings it to the device.  sa: the arguments both kernels share, but for the verdict records and gamma; gridX: the
// gathered downdate's.
int schUpload(eqf_filter* f, const SchCall& sc, const int* N, SchArgs& sa, int& gridX) {
    const int B = f->B;
    const schmidt::Image im{size_t(B), size_t(f->ld)};
    HIPC(f->sch.img.wait());
    std::vector<int> act;
    std::vector<unsigned char> fl;
    int nAmax = 0;
    for (int b = 0; b < B; ++b) {
        const int nc = sc.n ? sc.n[b] : 0;
        schmidt::buildActive(N[b], f->ids[b].data(), nc, nc ? sc.ids + size_t(b) * sc.cstride : nullptr, act, fl);
        schmidt::fillFilter(im, size_t(b), act, fl, f->sch.img.host);
        nAmax = std::max(nAmax, int(act.size()));
    }
    const int nMax = schmidt::paddedOrder(maxN(f));
    sa = SchArgs{};
    sa.g = f->g[f->pG]; sa.Sigma = static_cast<double*>(f->Sigma[f->pS]); sa.ld = f->ld; sa.sigmaStride = f->sigmaStride;
    sa.cnt = reinterpret_cast<const int*>(f->sch.img.dev + im.offCount()); sa.act = reinterpret_cast<const int*>(f->sch.img.dev + im.offActive());
    sa.flag = reinterpret_cast<const unsigned char*>(f->sch.img.dev + im.offFlag()); sa.pitch = f->ld; sa.nJT = schmidt::colTiles(nMax);
    sa.cntH = reinterpret_cast<const int*>(f->sch.img.host.dev + im.offCount()); sa.actH = reinterpret_cast<const int*>(f->sch.img.host.dev + im.offActive());
    sa.flagH = reinterpret_cast<const unsigned char*>(f->sch.img.host.dev + im.offFlag());
    sa.cntW = reinterpret_cast<int*>(f->sch.img.dev + im.offCount()); sa.actW = reinterpret_cast<int*>(f->sch.img.dev + im.offActive());
    sa.flagW = reinterpret_cast<unsigned char*>(f->sch.img.dev + im.offFlag());
    gridX = schmidt::gridX(nAmax, nMax);
    return EQF_OK;
}
// (sch.img's event: the pinned image has been read)
int schGammaLaunch(eqf_filter* f, const SchArgs& sa) {
    hipLaunchKernelGGL(k_schmidt_gamma, dim3((f->ld + 255) / 256, f->B), dim3(256), 0, f->stream, sa);
    HIPC(f->sch.img.record(f->stream));
    return EQF_OK;
}

// ---- the closing stage of every call that leaves an increment on the device: eqf_update_linear, eqf_update_landmarks and their variants
// behind the solve, eqf_apply_increment and eqf_perturb_filters behind their upload or draw
struct IncCall {
    double* gamma;              // filter b's increment: gamma[b * strideG + j] is internal index off + j
    long long strideG;
    int off;
    const unsigned char* mask;  // device [B], 0 leaves a filter alone; nullptr: none
    double* verdict;            // records [B][kLinHead] whose entry 3 the lift and the group step obey; nullptr: none
    bool liftRefuses;           // ... an update's: a lift that fails writes its refusal there
    const SchCall* sch;         // the Schmidt stage: nullptr, or the consider lists (checked; schReserve has run) ...
    const int* N;               // ... and every filter's landmark count
};
// Enqueues: the Schmidt partition and k_schmidt_gamma where the call has consider lists (in front of the lift and the group step: they see
// the masked gamma); the lift (it reads the Sigma the call started from and may still refuse a filter: in front of the downdate); the
// route's downdate -- downdate(sa, gridX) -> rc, sa the Schmidt arguments and gridX the gathered downdate's grid, or nullptr and 0 --;
// the group step, behind the verdict.  (liftReserve has run.)
extern "C++" template <class Downdate>  // (this part of the file lies inside the C ABI's linkage block)
int closeIncrement(eqf_filter* f, const IncCall& c, Downdate&& downdate) {
    SchArgs sa{};
    int schGrid = 0;
    if (c.sch) {
        int rc = schUpload(f, *c.sch, c.N, sa, schGrid);
        if (rc) return rc;
        sa.out = c.verdict; sa.gamma = c.gamma; sa.strideG = c.strideG;
        rc = schGammaLaunch(f, sa);
        if (rc) return rc;
    }
    IncArgs ia{};
    ia.g = f->g[f->pG]; ia.p0 = f->p0; ia.Q = f->Q[f->pG]; ia.cap = f->cap; ia.gamma = c.gamma; ia.strideG = c.strideG; ia.off = c.off;
    ia.mask = c.mask; ia.info = c.verdict;
    int rc = liftEnqueue(f, c.gamma, c.strideG, c.off, c.mask, c.verdict, c.liftRefuses, ia);
    if (!rc) rc = downdate(c.sch ? &sa : nullptr, schGrid);
    if (rc) return rc;
    hipLaunchKernelGGL(k_apply_increment, dim3(f->B), dim3(256), 0, f->stream, ia);
    HIPC(hipGetLastError());
    f->csValid = false;  // (C Sigma / S left by an earlier burst describe the old Sigma and the landmarks as they were)
    return EQF_OK;
}
constexpr auto noDowndate = [](const SchArgs*, int) { return int(EQF_OK); };  // (a call that leaves Sigma alone)
}  // namespace

int eqf_get_lift_report(eqf_filter* f, int b, eqf_lift_report* out) {
    if (!f || !out || b < 0 || b >= f->B || !f->lift.called) return EQF_ERR_INVALID;
    double rec[kLiftRec];
    HIPC(hipMemcpyAsync(rec, f->lift.rec + size_t(b) * kLiftRec, sizeof(rec), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    lift::Report r;
    lift::unpackReport(rec, &r);
    out->kind = r.kind;
    out->info = r.info;
    std::copy(r.DeltaU, r.DeltaU + 6, out->DeltaU);
    out->min_pivot = r.min_pivot;
    out->pivot_ratio = r.pivot_ratio;
    return EQF_OK;
}

// ---- draws from the covariance and the group step (eqf_sample.hpp; index arithmetic and argument checks: eqf_sample_host.hpp)
namespace {
sample::SmallLayout sampSmall(const eqf_filter* f) { return {size_t(f->B), size_t(f->cap)}; }
// one side of the staged image (sample::SmallLayout)
struct SampSmall {
    double *scale, *vec;
    unsigned char* mask;
};
SampSmall sampSide(const eqf_filter* f, char* p) {
    const sample::SmallLayout sl = sampSmall(f);
    double* d = reinterpret_cast<double*>(p);
    return SampSmall{d + sl.offScale(), d + sl.offVec(), reinterpret_cast<unsigned char*>(d + sl.offMask())};
}
// the small operands as a staged image
int sampSmallReserve(eqf_filter* f) {
    const workspace::Want w[] = {WANT_STAGED(f->samp.small, sampSmall(f).bytes())};
    return reserveSlots(f, w);
}
// room for `rows` samples per filter
int sampRowsReserve(eqf_filter* f, int rows) {
    const size_t bytes = sizeof(double) * size_t(rows) * f->ld * f->B;
    const workspace::Want w[] = {want(f->samp.Z, bytes, &f->samp.cap), want(f->samp.E, bytes, &f->samp.cap)};
    return reserveSlots(f, w);
}
// E = scale Z L^T behind neesFactor (nsamp >= 1 rows per filter in samp.Z -> samp.E, row pitch ldE)
void sampTrmm(eqf_filter* f, int off, int nsamp, int ldE, const double* dScale) {
    const int mMax = sample::paddedOrder(maxN(f), off);
    if (mMax <= 0) return;
    SampleArgs s{};
    s.g = f->g[f->pG]; s.A = f->dSigmaLoc; s.ld = f->ld; s.strideA = f->sigmaStride; s.Z = f->samp.Z; s.E = f->samp.E; s.ldE = ldE;
    s.nsamp = nsamp; s.scale = dScale; s.off = off;
    hipLaunchKernelGGL(k_sample_trmm, dim3(sample::blockColumns(mMax), sample::rowTiles(nsamp), f->B), dim3(256), kSampleLdsBytes, f->stream, s);
}
}  // namespace

int eqf_sample_sigma(eqf_filter* f, int local, int first, int nsamp, const double* z, int ldz, const double* scale, double* eps, int lde,
    eqf_sigma_stats* stats) {
    if (!f) return EQF_ERR_INVALID;
    // (the landmark counts are only known for certain behind GATE: the arguments that do not depend on them first, the strides after it)
    if (!sample::drawArgsOk(local, first, nsamp, z, ldz, eps, lde, stats, 0)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int B = f->B, nMax = maxN(f);
    if (!sample::drawArgsOk(local, first, nsamp, z, ldz, eps, lde, stats, nMax)) return EQF_ERR_INVALID;
    int rc = neesReserve(f);
    if (!rc && nsamp > 0) rc = sampRowsReserve(f, nsamp);
    if (!rc && scale) rc = sampSmallReserve(f);
    if (rc) return rc;
    const int off = sample::cutOffset(first), ldE = std::max(sample::paddedOrder(nMax, off), 1);
    rc = neesFactor(f, local, off, 0);
    if (rc) return rc;
    std::vector<double> hZ;
    if (nsamp > 0) {
        hZ.resize(size_t(B) * nsamp * ldE);
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < nsamp; ++k)
                sample::packRow(z + (size_t(b) * nsamp + k) * ldz, first, int(f->ids[b].size()), hZ.data() + (size_t(b) * nsamp + k) * ldE, ldE);
        HIPC(hipMemcpyAsync(f->samp.Z, hZ.data(), sizeof(double) * hZ.size(), hipMemcpyHostToDevice, f->stream));
        const double* dScale = nullptr;
        if (scale) {
            HIPC(f->samp.small.wait());
            SampSmall h = sampSide(f, f->samp.small.host), d = sampSide(f, f->samp.small.dev);
            std::copy(scale, scale + B, h.scale);
            const sample::Range r = sampSmall(f).scaleRange();
            HIPC(f->samp.small.upload(r.bytes, f->stream, r.offset));
            dScale = d.scale;
        }
        sampTrmm(f, off, nsamp, ldE, dScale);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(hZ.data(), f->samp.E, sizeof(double) * hZ.size(), hipMemcpyDeviceToHost, f->stream));
    }
    std::vector<double> hO;
    rc = readNeesRecords(f, hO);
    if (rc) return rc;
    if (stats) neesStats(hO.data(), B, stats);
    const double nan = std::nan("");
    const sample::RecordsLayout rl{size_t(B)};
    for (int b = 0; b < B; ++b) {
        const bool bad = hO[rl.offInfo(b)] != 0.0;
        for (int k = 0; k < nsamp; ++k)
            sample::unpackRow(hZ.data() + (size_t(b) * nsamp + k) * ldE, first, int(f->ids[b].size()), eps + (size_t(b) * nsamp + k) * lde,
                bad ? &nan : nullptr);
    }
    return EQF_OK;
}

int eqf_apply_increment(eqf_filter* f, const double* gamma, int ldg, const unsigned char* mask) {
    if (!f || !gamma) return EQF_ERR_INVALID;
    GATE(f);
    const int B = f->B;
    const std::vector<int> N = landmarkCounts(f);
    if (!sample::incrementArgsOk(gamma, ldg, mask, B, N.data())) return EQF_ERR_INVALID;
    int rc = sampSmallReserve(f);
    if (!rc) rc = liftReserve(f, lift::callFactors(liftCallKind(f), maxN(f)));
    if (rc) return rc;
    HIPC(f->samp.small.wait());
    SampSmall h = sampSide(f, f->samp.small.host), d = sampSide(f, f->samp.small.dev);
    const int len = int(sampSmall(f).vecLen());
    for (int b = 0; b < B; ++b) {
        sample::packRow(gamma + size_t(b) * ldg, 0, N[b], h.vec + size_t(b) * len, kLm0 + 3 * N[b]);
        h.mask[b] = mask ? mask[b] : 1;
    }
    const sample::Range r = sampSmall(f).vecMaskRange();
    HIPC(f->samp.small.upload(r.bytes, f->stream, r.offset));
    return closeIncrement(f, IncCall{d.vec, len, 0, d.mask, nullptr, false, nullptr, nullptr}, noDowndate);
}

int eqf_perturb_filters(eqf_filter* f, int first, const double* z, int ldz, const double* scale, eqf_sigma_stats* stats) {
    if (!f || !sample::perturbArgsOk(first, z, ldz, scale, f->B, 0)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int B = f->B, nMax = maxN(f);
    if (!sample::perturbArgsOk(first, z, ldz, scale, B, nMax)) return EQF_ERR_INVALID;
    int rc = neesReserve(f);
    if (!rc) rc = sampRowsReserve(f, 1);
    if (!rc) rc = sampSmallReserve(f);
    if (!rc) rc = liftReserve(f, lift::callFactors(liftCallKind(f), nMax));
    if (rc) return rc;
    const int off = sample::cutOffset(first), ldE = std::max(sample::paddedOrder(nMax, off), 1);
    rc = neesFactor(f, 0, off, 0);
    if (rc) return rc;
    HIPC(f->samp.small.wait());
    SampSmall h = sampSide(f, f->samp.small.host), d = sampSide(f, f->samp.small.dev);
    for (int b = 0; b < B; ++b) {
        h.scale[b] = scale ? scale[b] : 1.0;
        h.mask[b] = h.scale[b] != 0.0;
        sample::packRow(z + size_t(b) * ldz, first, int(f->ids[b].size()), h.vec + size_t(b) * ldE, ldE);
    }
    HIPC(hipMemcpyAsync(d.scale, h.scale, sizeof(double) * B, hipMemcpyHostToDevice, f->stream));
    HIPC(hipMemcpyAsync(d.mask, h.mask, size_t(B), hipMemcpyHostToDevice, f->stream));
    HIPC(hipMemcpyAsync(f->samp.Z, h.vec, sizeof(double) * size_t(B) * ldE, hipMemcpyHostToDevice, f->stream));
    HIPC(f->samp.small.record(f->stream));
    // (a submatrix of order 0 -- first = 11, no landmarks anywhere -- has no sample: k_apply_increment then reads no entry of the image)
    sampTrmm(f, off, 1, ldE, d.scale);
    // (the lift factors Sigma[6:, 6:] in the scratch image: the draw's factor has been consumed by sampTrmm; the draw's records are the verdict)
    rc = closeIncrement(f, IncCall{f->samp.E, ldE, off, d.mask, f->nees.out, false, nullptr, nullptr}, noDowndate);
    if (rc) return rc;
    if (!stats) return EQF_OK;
    std::vector<double> hO;
    rc = readNeesRecords(f, hO);
    if (rc) return rc;
    neesStats(hO.data(), B, stats);
    return EQF_OK;
}

// ---- the low-rank linear measurement update (eqf_linear.hpp; index arithmetic and argument checks: eqf_linear_host.hpp)
static_assert(linear::kRefBase == kBase && linear::kPadBase == kLm0 && linear::kRows == kLinRows && linear::kTile == kSB &&
              linear::kHead == kLinHead, "eqf_linear_host.hpp repeats the layout constants");
namespace {
// every buffer of eqf_update_linear, from capacity and batch
int linReserve(eqf_filter* f) {
    const linear::SmallLayout sl{f->B, linear::refOrder(f->cap)};
    const linear::WorkLayout wl{f->ld};
    const workspace::Want w[] = {WANT_STAGED(f->lin.small, sl.bytes()), want(f->lin.ws, sizeof(double) * size_t(wl.stride()) * f->B),
        want(f->lin.out, sizeof(double) * size_t(kLinHead) * f->B)};
    return reserveSlots(f, w);
}

// eqf_update_linear (sc == nullptr: the launches it has always enqueued) and eqf_update_linear_schmidt
int linUpdate(eqf_filter* f, int local, int m, const double* H, int ldh, const double* resid, const double* R, double gate,
    const unsigned char* mask, const SchCall* sc, double* gamma, int ldg, eqf_linear_report* report) {
    if (!f || !linear::headArgsOk(local, m, H, resid, R, gate)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);  // (queued IMU calls and a pending gate first: the gate may still change the landmark counts)
    const int B = f->B;
    const std::vector<int> N = landmarkCounts(f);
    if (!linear::argsOk(m, H, ldh, resid, R, mask, gamma, ldg, B, N.data())) return EQF_ERR_INVALID;
    if (sc) {
        const int bad = schmidt::checkLists(B, f->cap, sc->n, sc->ids, sc->cstride);
        if (bad) return bad;
    }
    int rc = linReserve(f);
    if (!rc && sc) rc = schReserve(f);
    if (!rc) rc = liftReserve(f, lift::callFactors(liftCallKind(f), maxN(f)));
    if (rc) return rc;
    if (local) {
        rc = launchLocal(f, 0, B, false);  // (only writes the J records)
        if (rc) return rc;
    }
    const linear::SmallLayout sl{B, linear::refOrder(f->cap)};
    const linear::WorkLayout wl{f->ld};
    HIPC(f->lin.small.wait());
    double* hs = reinterpret_cast<double*>(f->lin.small.host.get());
    double* ds = reinterpret_cast<double*>(f->lin.small.dev.get());
    unsigned char* hm = reinterpret_cast<unsigned char*>(hs + sl.offMask());
    for (int b = 0; b < B; ++b) {
        linear::packFilter(m, N[b], H + size_t(b) * m * ldh, ldh, resid + size_t(b) * m, R + size_t(b) * m * m,
            hs + sl.offH() + size_t(b) * kLinRows * sl.ldr, sl.ldr, hs + sl.offResid() + size_t(b) * kLinRows,
            hs + sl.offR() + size_t(b) * kLinRows * kLinRows);
        hm[b] = mask ? (mask[b] ? 1 : 0) : 1;
    }
    HIPC(f->lin.small.upload(sl.bytes(), f->stream));
    const int nMax = maxN(f), nt = linear::rowTiles(nMax);
    LinArgs a{};
    a.g = f->g[f->pG]; a.Sigma = static_cast<double*>(f->Sigma[f->pS]); a.ld = f->ld; a.sigmaStride = f->sigmaStride;
    a.H = ds + sl.offH(); a.ldr = sl.ldr; a.resid = ds + sl.offResid(); a.R = ds + sl.offR();
    a.mask = reinterpret_cast<const unsigned char*>(ds + sl.offMask());
    a.jac = local ? f->dJac : nullptr; a.cap = f->cap; a.m = m; a.gate = gate;
    a.ws = f->lin.ws; a.wsStride = wl.stride(); a.out = f->lin.out;
    rc = profiled(f, EQF_PROF_LIN_ROWS, [&] { hipLaunchKernelGGL(k_lin_rows, dim3(B), dim3(256), 0, f->stream, a); });
    if (!rc) rc = profiled(f, EQF_PROF_LIN_GAIN, [&] { hipLaunchKernelGGL(k_lin_gain, dim3(nt, B), dim3(256), kLinGainLdsBytes, f->stream, a); });
    if (!rc) rc = profiled(f, EQF_PROF_LIN_SOLVE, [&] { hipLaunchKernelGGL(k_lin_solve, dim3(B), dim3(256), 0, f->stream, a); });
    if (rc) return rc;
    // the group step obeys the solve's verdict (entry 3 of the record, where eqf_nees.hpp's info sits)
    rc = closeIncrement(f, IncCall{f->lin.ws + wl.offGamma(), wl.stride(), 0, nullptr, f->lin.out, true, sc, N.data()},
        [&](const SchArgs* sa, int schGrid) {
            if (!sa)
                return profiled(f, EQF_PROF_LIN_DOWNDATE,
                    [&] { hipLaunchKernelGGL(k_lin_downdate, dim3(linear::triTiles(nt), B), dim3(256), 0, f->stream, a); });
            const SchLin lay{f->lin.ws + wl.offY(), wl.stride(), f->ld};
            return profiled(f, EQF_PROF_LIN_DOWNDATE, [&] {
                hipLaunchKernelGGL(k_schmidt_downdate<SchLin>, dim3(schGrid, B), dim3(256), schmidtLdsBytes<SchLin>(), f->stream, *sa, lay);
            });
        });
    if (rc) return rc;
    if (!gamma && !report) return EQF_OK;
    std::vector<double> hO(size_t(B) * kLinHead), hG;
    HIPC(hipMemcpyAsync(hO.data(), f->lin.out, sizeof(double) * hO.size(), hipMemcpyDeviceToHost, f->stream));
    if (gamma) {
        hG.resize(size_t(B) * f->ld);
        HIPC(hipMemcpy2DAsync(hG.data(), sizeof(double) * f->ld, f->lin.ws + wl.offGamma(), sizeof(double) * wl.stride(),
            sizeof(double) * f->ld, B, hipMemcpyDeviceToHost, f->stream));
    }
    HIPC(hipStreamSynchronize(f->stream));
    for (int b = 0; b < B; ++b) {
        const double* o = hO.data() + size_t(b) * kLinHead;
        if (report) report[b] = linearReport(lift::updateReport(o, m, false));
        if (gamma) linear::unpackGamma(hG.data() + size_t(b) * f->ld, N[b], gamma + size_t(b) * ldg, int(o[3]) != 0);
    }
    return EQF_OK;
}
}  // namespace

int eqf_update_linear(eqf_filter* f, int local, int m, const double* H, int ldh, const double* resid, const double* R, double gate,
    const unsigned char* mask, double* gamma, int ldg, eqf_linear_report* report) {
    return linUpdate(f, local, m, H, ldh, resid, R, gate, mask, nullptr, gamma, ldg, report);
}
int eqf_update_linear_schmidt(eqf_filter* f, int local, int m, const double* H, int ldh, const double* resid, const double* R, double gate,
    const unsigned char* mask, const int* n_consider, const int* consider_ids, int cstride, double* gamma, int ldg,
    eqf_linear_report* report) {
    const SchCall sc{n_consider, consider_ids, cstride};
    return linUpdate(f, local, m, H, ldh, resid, R, gate, mask, &sc, gamma, ldg, report);
}

// ---- the per-landmark block measurement update (eqf_blocks.hpp; per-entry arithmetic, index arithmetic and argument checks:
// eqf_blocks_host.hpp)
static_assert(blocks::kRefBase == kBase && blocks::kPadBase == kLm0 && blocks::kTile == kSB && blocks::kHead == kLinHead,
    "eqf_blocks_host.hpp repeats the layout constants");
namespace {
// what eqf_observe_landmarks hands the call in place of rows
struct ObsCall {
    int kind;
    const double* cam;
    int camPerFilter;
    const double* meas;
    double* HtOut;
    double* residOut;
};
// what eqf_observe_landmarks_iterated adds to that
struct IterCall {
    int maxLin;
    double tol;
    double* gTrace;
    eqf_iter_report* rep;
};
// One call of the route as its four entry points fill it: eqf_update_landmarks (sch, obs, iter nullptr: the launches it has always
// enqueued), eqf_update_landmarks_schmidt (sch), eqf_observe_landmarks (obs: local = 0, Hb and resid nullptr -- k_obs_rows forms the rows on
// the device in k_blk_rows's place) and eqf_observe_landmarks_iterated (obs and iter: with more than one linearisation the kernels of
// eqf_iterate.hpp run between k_obs_rows and k_blk_gain and leave the committed rows where k_obs_rows left its own)
struct BlkCall {
    int local, rows;
    const int *nk, *ids;
    int stride;
    const double *Hb, *resid, *Rb;
    double gate, lmGate;
    const unsigned char* mask;
    const SchCall* sch;
    const ObsCall* obs;
    const IterCall* iter;
    unsigned char* used;
    double* gamma;
    int ldg;
    eqf_linear_report* report;
};
// What the call's shape decides, once, behind the checks: the layouts; where the operands both kinds of image hold lie in this call's
// (observe::SmallLayout with obs, blocks::SmallLayout without); whether intermediate linearisations run; the bytes of the image and of the
// rows array (two of them when iterating, none without obs); the grids' tile counts
struct BlkPlan {
    blocks::SmallLayout sl;
    observe::SmallLayout ol;
    observe::RowsLayout orl;
    blocks::WorkLayout wl;
    iterate::WorkLayout il;
    bool iterating;
    size_t smallBytes, obsBytes, offR, offIdx, offNk, offMask;
    int nMax, nt, nPT;
};
BlkPlan blkPlan(const eqf_filter* f, const BlkCall& c) {
    BlkPlan p{{f->B, c.stride, c.rows}, {f->B, c.stride, c.rows}, {f->B, c.stride, c.rows}, {f->ld, c.stride, c.rows, kDRec},
        {c.stride, c.rows, kDRec}};
    p.iterating = c.iter && c.iter->maxLin > 1;
    p.smallBytes = p.iterating ? iterate::smallBytes(p.ol) : (c.obs ? p.ol.bytes() : p.sl.bytes());
    p.obsBytes = c.obs ? sizeof(double) * p.orl.doubles() * (p.iterating ? 2 : 1) : 0;
    p.offR = c.obs ? p.ol.offR() : p.sl.offR(); p.offIdx = c.obs ? p.ol.offIdx() : p.sl.offIdx();
    p.offNk = c.obs ? p.ol.offNk() : p.sl.offNk(); p.offMask = c.obs ? p.ol.offMask() : p.sl.offMask();
    p.nMax = maxN(f); p.nt = blocks::rowTiles(p.nMax); p.nPT = blocks::pairTiles(c.stride);
    return p;
}

// The argument checks.  Behind GATE (queued IMU calls and a pending gate first: the gate may still change the landmark lists) N holds the
// landmark counts.
int blkCheck(eqf_filter* f, const BlkCall& c, std::vector<int>& N) {
    if (!f) return EQF_ERR_INVALID;
    const ObsCall* oc = c.obs;
    if (c.iter && !iterate::argsOk(c.iter->maxLin, c.iter->tol)) return EQF_ERR_INVALID;
    if (oc ? !observe::headArgsOk(oc->kind, oc->camPerFilter, c.nk, c.ids, c.stride, oc->meas, c.Rb, c.gate, c.lmGate)
           : !blocks::headArgsOk(c.local, c.rows, c.nk, c.ids, c.stride, c.Hb, c.resid, c.Rb, c.gate, c.lmGate))
        return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    const int B = f->B;
    N = landmarkCounts(f);
    const int bad = oc ? observe::argsCheck(oc->kind, oc->cam, oc->camPerFilter, c.nk, c.ids, c.stride, oc->meas, c.Rb, c.mask, c.gamma, c.ldg, B,
                             N.data(), f->cap)
                       : blocks::argsCheck(c.rows, c.nk, c.ids, c.stride, c.Hb, c.resid, c.Rb, c.mask, c.gamma, c.ldg, B, N.data(), f->cap);
    if (bad) return bad == 1 ? EQF_ERR_INVALID : (bad == 2 ? EQF_ERR_UNSORTED : EQF_ERR_CAPACITY);
    return c.sch ? schmidt::checkLists(B, f->cap, c.sch->n, c.sch->ids, c.sch->cstride) : int(EQF_OK);
}

// Every buffer of the call for its shape -- its own, the intermediate linearisations', the lift's, the Schmidt partition's; what is there
// and large enough is kept -- and the dynamic LDS of its two downdates
int blkReserve(eqf_filter* f, const BlkCall& c, const BlkPlan& p) {
    const size_t B = size_t(f->B);
    const workspace::Want w[] = {WANT_STAGED(f->blk.small, p.smallBytes), want(f->blk.ws, sizeof(double) * size_t(p.wl.strideD()) * B, &f->blk.wsCap),
        want(f->blk.wi, sizeof(int) * size_t(p.wl.strideI()) * B, &f->blk.wiCap), want(f->blk.out, sizeof(double) * size_t(kLinHead) * B),
        want(f->blk.obs, p.obsBytes, &f->blk.obsCap)};
    int rc = reserveSlots(f, w);
    if (!rc && p.iterating) {
        const workspace::Want wi[] = {want(f->iter.ws, sizeof(double) * size_t(p.il.strideD()) * B, &f->iter.wsCap),
            want(f->iter.wi, sizeof(int) * size_t(iterate::WorkLayout::kInts) * B, &f->iter.wiCap),
            want(f->iter.trace, sizeof(double) * iterate::traceDoubles(c.iter->maxLin, f->B, c.stride), &f->iter.traceCap)};
        rc = reserveSlots(f, wi);
    }
    if (!rc) rc = liftReserve(f, lift::callFactors(liftCallKind(f), p.nMax));
    if (!rc && c.sch) rc = schReserve(f);
    if (!rc && c.sch) rc = allowRouteLds(f->sch.ldsSet, {{ldsFn(&k_schmidt_downdate<SchBlk>), int(schmidtLdsBytes<SchBlk>())}});
    if (!rc) rc = allowRouteLds(f->blk.downLdsSet, {{ldsFn(&k_blk_downdate), kBlkDownLdsBytes}});
    return rc;
}

// The call's operands into the pinned image and on their way to the device: the caller's arrays as they are, and per entry the landmark's
// index in its filter's state (-1: the id is not there, the entry lies beyond nk or the filter is masked out); when iterating, one byte per
// entry behind them: its landmark is a consider one
int blkPack(eqf_filter* f, const BlkCall& c, const BlkPlan& p, const int* N) {
    const int B = f->B, stride = c.stride, rows = c.rows;
    const ObsCall* oc = c.obs;
    const SchCall* sc = c.sch;
    HIPC(f->blk.small.wait());
    char* hs = f->blk.small.host;
    const size_t ne = p.sl.entries();
    if (oc) {
        double* hCam = reinterpret_cast<double*>(hs + p.ol.offCam());
        for (int b = 0; b < B; ++b) {
            const bool read = oc->cam && (!oc->camPerFilter || !c.mask || c.mask[b]);  // (a masked filter's own offset is never read)
            observe::unitCam(read ? oc->cam + (oc->camPerFilter ? size_t(b) * observe::kCam : 0) : nullptr, hCam + size_t(b) * observe::kCam);
        }
        std::memcpy(hs + p.ol.offMeas(), oc->meas, sizeof(double) * ne * 3);
    } else {
        std::memcpy(hs + p.sl.offH(), c.Hb, sizeof(double) * ne * rows * 3);
        std::memcpy(hs + p.sl.offResid(), c.resid, sizeof(double) * ne * rows);
    }
    std::memcpy(hs + p.offR, c.Rb, sizeof(double) * ne * rows * rows);
    int* hIdx = reinterpret_cast<int*>(hs + p.offIdx);
    int* hNk = reinterpret_cast<int*>(hs + p.offNk);
    unsigned char* hm = reinterpret_cast<unsigned char*>(hs + p.offMask);
    for (int b = 0; b < B; ++b) {
        hNk[b] = c.nk[b];
        hm[b] = c.mask ? (c.mask[b] ? 1 : 0) : 1;
        for (int k = 0; k < stride; ++k)
            hIdx[size_t(b) * stride + k] = (hm[b] && k < c.nk[b]) ? blocks::findId(f->ids[b].data(), N[b], c.ids[size_t(b) * stride + k]) : -1;
        for (int k = 0; p.iterating && k < stride; ++k)
            hs[iterate::offConsider(p.ol) + size_t(b) * stride + k] = (sc && sc->n && hm[b] && k < c.nk[b] &&
                iterate::considered(sc->ids + size_t(b) * sc->cstride, sc->n[b], c.ids[size_t(b) * stride + k])) ? 1 : 0;
    }
    HIPC(f->blk.small.upload(p.smallBytes, f->stream));
    return EQF_OK;
}

// the arguments every kernel of the route takes: the rows where k_obs_rows forms them, or in the uploaded image
BlkArgs blkArgs(eqf_filter* f, const BlkCall& c, const BlkPlan& p) {
    const char* ds = f->blk.small.dev;
    BlkArgs a{};
    a.g = f->g[f->pG]; a.Sigma = static_cast<double*>(f->Sigma[f->pS]); a.ld = f->ld; a.sigmaStride = f->sigmaStride;
    if (c.obs) {
        a.Hb = f->blk.obs + p.orl.offHt(); a.resid = f->blk.obs + p.orl.offResid();
    } else {
        a.Hb = reinterpret_cast<const double*>(ds + p.sl.offH()); a.resid = reinterpret_cast<const double*>(ds + p.sl.offResid());
    }
    a.Rb = reinterpret_cast<const double*>(ds + p.offR); a.idx = reinterpret_cast<const int*>(ds + p.offIdx);
    a.nk = reinterpret_cast<const int*>(ds + p.offNk); a.mask = reinterpret_cast<const unsigned char*>(ds + p.offMask);
    a.jac = c.local ? f->dJac : nullptr; a.cap = f->cap; a.rows = c.rows; a.stride = c.stride; a.mp = p.wl.mp(); a.nb = p.wl.nb();
    a.gate = c.gate; a.lmGate = c.lmGate;
    a.ws = f->blk.ws; a.wsStride = p.wl.strideD(); a.offHt = p.wl.offHt(); a.offGamma = p.wl.offGamma(); a.offD = p.wl.offD();
    a.wi = f->blk.wi; a.wiStride = p.wl.strideI(); a.out = f->blk.out;
    return a;
}

// The intermediate linearisations behind k_obs_rows: per solve the form kernel, the factorisation, the step and the rows kernel; one commit
// behind them.  Every launch is counted (eqf_debug_iterate_launches).
int blkIterate(eqf_filter* f, const BlkCall& c, const BlkPlan& p, const ObsArgs& o) {
    const int B = f->B, maxLin = c.iter->maxLin;
    const iterate::WorkLayout& il = p.il;
    IterArgs t{};
    t.a = o.a; t.kind = o.kind; t.cam = o.cam; t.meas = o.meas; t.p0 = o.p0; t.Q = o.Q;
    t.consider = reinterpret_cast<const unsigned char*>(f->blk.small.dev + iterate::offConsider(p.ol));
    t.rowsBuf = f->blk.obs; t.bufStride = (long long)p.orl.doubles(); t.offResid = (long long)p.orl.offResid();
    t.ws = f->iter.ws; t.wsStride = il.strideD(); t.offT = il.offT(); t.offW = il.offW(); t.offG = il.offG(); t.offGn = il.offGn();
    t.offD = il.offD(); t.offStep = il.offStep(); t.wi = f->iter.wi; t.trace = f->iter.trace; t.maxLin = maxLin; t.B = B;
    t.tol = c.iter->tol;
    // the progress words, g, gNext and lastStep of every filter and the whole trace start as zeros
    HIPC(hipMemsetAsync(f->iter.wi, 0, sizeof(int) * size_t(iterate::WorkLayout::kInts) * B, f->stream));
    HIPC(hipMemset2DAsync(f->iter.ws + il.offG(), sizeof(double) * il.strideD(), 0, sizeof(double) * (il.strideD() - il.offG()), B, f->stream));
    HIPC(hipMemsetAsync(f->iter.trace, 0, sizeof(double) * iterate::traceDoubles(maxLin, B, c.stride), f->stream));
    for (int k = 0; k + 1 < maxLin; ++k) {
        hipLaunchKernelGGL(k_iter_form, dim3(p.nPT * p.nPT, B), dim3(256), 0, f->stream, t, p.nPT);
        const int rc = enqueueFactor(f->stream, f->iter.ldsSet, t, B, il.mp(), 1, &f->iter.launches);
        if (rc) return rc;
        hipLaunchKernelGGL(k_iter_step, dim3(B), dim3(256), 0, f->stream, t, k);
        hipLaunchKernelGGL(k_iter_rows, dim3(B), dim3(256), 0, f->stream, t, k);
        f->iter.launches += 3;
    }
    hipLaunchKernelGGL(k_iter_commit, dim3(B), dim3(256), 0, f->stream, t);
    ++f->iter.launches;
    return EQF_OK;
}
// The rows: the caller's through k_blk_rows, or formed at each filter's own estimate by k_obs_rows and, where the call iterates, re-formed
int blkFormRows(eqf_filter* f, const BlkCall& c, const BlkPlan& p, const BlkArgs& a) {
    if (!c.obs) {
        hipLaunchKernelGGL(k_blk_rows, dim3(f->B), dim3(256), 0, f->stream, a);
        return EQF_OK;
    }
    const char* ds = f->blk.small.dev;
    ObsArgs o{};
    o.a = a; o.kind = c.obs->kind; o.cam = reinterpret_cast<const double*>(ds + p.ol.offCam());
    o.meas = reinterpret_cast<const double*>(ds + p.ol.offMeas()); o.p0 = f->p0; o.Q = f->Q[f->pG];
    o.Ht = f->blk.obs + p.orl.offHt(); o.resid = f->blk.obs + p.orl.offResid();
    hipLaunchKernelGGL(k_obs_rows, dim3(f->B), dim3(256), 0, f->stream, o);
    if (c.iter) f->iter.launches = 0;
    return p.iterating ? blkIterate(f, c, p, o) : int(EQF_OK);
}
// the solve: gain, factorisation, gamma and the tail, which leaves every filter's verdict
int blkSolve(eqf_filter* f, const BlkPlan& p, const BlkArgs& a) {
    const int B = f->B;
    hipLaunchKernelGGL(k_blk_gain, dim3(p.nt + p.nPT * p.nPT, B), dim3(256), 0, f->stream, a, p.nt, p.nPT);
    const int rc = enqueueFactor(f->stream, f->blk.ldsSet, a, B, p.wl.mp(), blocks::rhsBlocks(blocks::paddedOrder(p.nMax)));
    if (rc) return rc;
    hipLaunchKernelGGL(k_blk_gamma, dim3(p.nt, B), dim3(64), 0, f->stream, a);
    hipLaunchKernelGGL(k_blk_tail, dim3(B), dim3(256), 0, f->stream, a);
    return EQF_OK;
}

// What the caller asked to see, behind the device: enqueues and returns where that is nothing
int blkReadBack(eqf_filter* f, const BlkCall& c, const BlkPlan& p, const int* N) {
    const ObsCall* oc = c.obs;
    const IterCall* ic = c.iter;
    const blocks::WorkLayout& wl = p.wl;
    const int B = f->B, stride = c.stride, rows = c.rows;
    if (!c.used && !c.gamma && !c.report && !(oc && (oc->HtOut || oc->residOut)) && !(ic && (ic->gTrace || ic->rep))) return EQF_OK;
    std::vector<double> hO(size_t(B) * kLinHead), hG, hRows, hStep;
    std::vector<int> hU(size_t(B) * wl.strideI()), hIt;
    if (p.iterating && ic->rep) {
        hStep.resize(B);
        hIt.resize(size_t(B) * iterate::WorkLayout::kInts);
        HIPC(hipMemcpyAsync(hIt.data(), f->iter.wi, sizeof(int) * hIt.size(), hipMemcpyDeviceToHost, f->stream));
        HIPC(hipMemcpy2DAsync(hStep.data(), sizeof(double), f->iter.ws + p.il.offStep(), sizeof(double) * p.il.strideD(), sizeof(double), B,
            hipMemcpyDeviceToHost, f->stream));
    }
    if (p.iterating && ic->gTrace)
        HIPC(hipMemcpyAsync(ic->gTrace, f->iter.trace, sizeof(double) * iterate::traceDoubles(ic->maxLin, B, stride), hipMemcpyDeviceToHost,
            f->stream));
    if (oc && (oc->HtOut || oc->residOut)) {
        hRows.resize(p.orl.doubles());
        HIPC(hipMemcpyAsync(hRows.data(), f->blk.obs, sizeof(double) * hRows.size(), hipMemcpyDeviceToHost, f->stream));
    }
    HIPC(hipMemcpyAsync(hO.data(), f->blk.out, sizeof(double) * hO.size(), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipMemcpyAsync(hU.data(), f->blk.wi, sizeof(int) * hU.size(), hipMemcpyDeviceToHost, f->stream));
    if (c.gamma) {
        hG.resize(size_t(B) * f->ld);
        HIPC(hipMemcpy2DAsync(hG.data(), sizeof(double) * f->ld, f->blk.ws + wl.offGamma(), sizeof(double) * wl.strideD(),
            sizeof(double) * f->ld, B, hipMemcpyDeviceToHost, f->stream));
    }
    HIPC(hipStreamSynchronize(f->stream));
    if (ic && ic->gTrace && !p.iterating) std::fill(ic->gTrace, ic->gTrace + iterate::traceDoubles(1, B, stride), 0.0);
    for (int b = 0; b < B; ++b) {
        const double* o = hO.data() + size_t(b) * kLinHead;
        const int* u = hU.data() + size_t(b) * wl.strideI();
        const int word = int(o[3]), cnt = word == 3 ? 0 : u[wl.offCount()];
        if (c.report) c.report[b] = linearReport(lift::updateReport(o, rows * cnt, true));
        if (c.used)
            for (int k = 0; k < stride; ++k) c.used[size_t(b) * stride + k] = (word != 3 && k < c.nk[b]) ? (unsigned char)u[wl.offUsed() + k] : 0;
        if (c.gamma) blocks::unpackGamma(hG.data() + size_t(b) * f->ld, N[b], c.gamma + size_t(b) * c.ldg, word != 0);
        if (ic && ic->rep) {
            using W = iterate::WorkLayout;  // (the filter's progress words; none without an intermediate solve)
            const iterate::Report r = p.iterating ? iterate::Report{hIt[size_t(b) * W::kInts + W::kNLin], hIt[size_t(b) * W::kInts + W::kStatus], hStep[b]}
                                                  : iterate::singleReport(word);
            ic->rep[b] = eqf_iter_report{r.n_lin, r.status, r.last_step};
        }
        for (int k = 0; oc && k < stride; ++k) {  // (the kernel stores zeros for an entry that is absent or not observable)
            const size_t e = size_t(b) * stride + k;
            const bool formed = word != 3 && k < c.nk[b];
            for (int q = 0; oc->HtOut && q < 3 * rows; ++q) oc->HtOut[e * rows * 3 + q] = formed ? hRows[p.orl.offHt() + e * rows * 3 + q] : 0.0;
            for (int q = 0; oc->residOut && q < rows; ++q) oc->residOut[e * rows + q] = formed ? hRows[p.orl.offResid() + e * rows + q] : 0.0;
        }
    }
    return EQF_OK;
}

int blkUpdate(eqf_filter* f, const BlkCall& c) {
    std::vector<int> N;
    int rc = blkCheck(f, c, N);
    if (rc) return rc;
    const BlkPlan p = blkPlan(f, c);
    rc = blkReserve(f, c, p);
    if (!rc && c.local) rc = launchLocal(f, 0, f->B, false);  // (only writes the J records)
    if (!rc) rc = blkPack(f, c, p, N.data());
    if (rc) return rc;
    const BlkArgs a = blkArgs(f, c, p);
    rc = blkFormRows(f, c, p, a);
    if (!rc) rc = blkSolve(f, p, a);
    if (rc) return rc;
    // the group step obeys the tail's verdict (entry 3 of the record, where eqf_nees.hpp's info sits)
    rc = closeIncrement(f, IncCall{f->blk.ws + p.wl.offGamma(), p.wl.strideD(), 0, nullptr, f->blk.out, true, c.sch, N.data()},
        [&](const SchArgs* sa, int schGrid) {
            if (sa) {
                const SchBlk lay{f->blk.ws, p.wl.strideD(), p.wl.mp(), c.rows, f->blk.wi + p.wl.offCount(), p.wl.strideI()};
                hipLaunchKernelGGL(k_schmidt_downdate<SchBlk>, dim3(schGrid, f->B), dim3(256), schmidtLdsBytes<SchBlk>(), f->stream, *sa, lay);
            } else {
                hipLaunchKernelGGL(k_blk_downdate, dim3(blocks::triTiles(p.nt), f->B), dim3(256), kBlkDownLdsBytes, f->stream, a);
            }
            return int(EQF_OK);
        });
    return rc ? rc : blkReadBack(f, c, p, N.data());
}
}  // namespace

int eqf_update_landmarks(eqf_filter* f, int local, int rows, const int* nk, const int* ids, int stride, const double* Hb, const double* resid,
    const double* Rb, double gate, double lm_gate, const unsigned char* mask, unsigned char* used, double* gamma, int ldg,
    eqf_linear_report* report) {
    return blkUpdate(f, BlkCall{local, rows, nk, ids, stride, Hb, resid, Rb, gate, lm_gate, mask, nullptr, nullptr, nullptr, used, gamma, ldg, report});
}
int eqf_update_landmarks_schmidt(eqf_filter* f, int local, int rows, const int* nk, const int* ids, int stride, const double* Hb,
    const double* resid, const double* Rb, double gate, double lm_gate, const unsigned char* mask, const int* n_consider,
    const int* consider_ids, int cstride, unsigned char* used, double* gamma, int ldg, eqf_linear_report* report) {
    const SchCall sc{n_consider, consider_ids, cstride};
    return blkUpdate(f, BlkCall{local, rows, nk, ids, stride, Hb, resid, Rb, gate, lm_gate, mask, &sc, nullptr, nullptr, used, gamma, ldg, report});
}
// the rows formed on the device (eqf_observe.hpp; per-entry arithmetic, layouts and argument checks: eqf_observe_host.hpp)
static_assert(observe::kBearing == EQF_OBS_BEARING && observe::kRange == EQF_OBS_RANGE && observe::kPosition == EQF_OBS_POSITION,
    "eqf_observe_host.hpp repeats the kinds");
int eqf_observe_landmarks(eqf_filter* f, int kind, const double* cam, int cam_per_filter, const int* nk, const int* ids, int stride,
    const double* meas, const double* Rb, double gate, double lm_gate, const unsigned char* mask, const int* n_consider,
    const int* consider_ids, int cstride, unsigned char* used, double* Ht_out, double* resid_out, double* gamma, int ldg,
    eqf_linear_report* report) {
    const ObsCall oc{kind, cam, cam_per_filter, meas, Ht_out, resid_out};
    const SchCall sc{n_consider, consider_ids, cstride};
    return blkUpdate(f, BlkCall{0, observe::rowsOf(kind), nk, ids, stride, nullptr, nullptr, Rb, gate, lm_gate, mask, n_consider ? &sc : nullptr, &oc,
                            nullptr, used, gamma, ldg, report});
}
// ... and re-formed at the moved estimate until the increment settles (eqf_iterate.hpp; eqf_iterate_host.hpp)
static_assert(iterate::kMaxLin == EQF_ITER_MAX_LIN, "eqf_iterate_host.hpp repeats the limit");
int eqf_observe_landmarks_iterated(eqf_filter* f, int kind, const double* cam, int cam_per_filter, const int* nk, const int* ids, int stride,
    const double* meas, const double* Rb, double gate, double lm_gate, const unsigned char* mask, const int* n_consider,
    const int* consider_ids, int cstride, int max_lin, double tol, unsigned char* used, double* Ht_out, double* resid_out, double* gamma,
    int ldg, eqf_linear_report* report, double* g_trace, eqf_iter_report* iter_report) {
    const ObsCall oc{kind, cam, cam_per_filter, meas, Ht_out, resid_out};
    const SchCall sc{n_consider, consider_ids, cstride};
    const IterCall ic{max_lin, tol, g_trace, iter_report};
    return blkUpdate(f, BlkCall{0, observe::rowsOf(kind), nk, ids, stride, nullptr, nullptr, Rb, gate, lm_gate, mask, n_consider ? &sc : nullptr, &oc,
                            &ic, used, gamma, ldg, report});
}

static_assert(mixture::kRefBase == kBase && mixture::kPadBase == kLm0 && mixture::kRows == kMixRows && mixture::kLanes == kMixLanes &&
              mixture::kEstHead == kMixEstHead && sizeof(mixture::Member) == sizeof(MixMember) && sizeof(Glob) % 8 == 0,
    "eqf_mixture_host.hpp repeats the layout constants");
namespace {
// every kernel launch of a mixture call is counted (eqf_debug_mixture_launches)
#define MIX_LAUNCH(f, ...)                  \
    do {                                    \
        hipLaunchKernelGGL(__VA_ARGS__);    \
        ++(f)->mix.launches;                 \
    } while (0)
constexpr int kMixGlobWords = int(sizeof(Glob) / 8);
// What both entry points check and build before any effect: the arguments, the members' landmark lists against the reference's, the
// normalised weights and the tables.  (GATE has run: the id lists are settled.)
struct MixCall {
    std::vector<double> wt;
    std::vector<mixture::Member> members;
    std::vector<int> uniq;
    double nEff = 0.0;
    int N = 0;
};
int mixCheck(eqf_filter* f, int n, const int* idx, const double* w, int ref, bool merge, MixCall& c) {
    const std::vector<int>& rid = f->ids[ref];
    for (int k = 0; k < n; ++k) {
        const int b = idx[k];
        if (!mixture::sameIds(f->ids[b].data(), int(f->ids[b].size()), rid.data(), int(rid.size()))) return EQF_ERR_INVALID;
        if (merge && (!f->init[b] || f->curTime[b] != f->curTime[ref])) return EQF_ERR_INVALID;
    }
    c.wt.resize(n);
    c.nEff = mixture::normalise(n, w, c.wt.data());
    mixture::buildTables(n, idx, c.wt.data(), ref, f->B, c.members, c.uniq);
    c.N = int(rid.size());
    return EQF_OK;  // (headArgsOk: the weight sum is positive, so at least one member is walked)
}
// every buffer a call needs: the workspace from capacity and batch, the table for this call's members
int mixReserve(eqf_filter* f, size_t tabBytes) {
    const mixture::WorkLayout wl{f->B, f->cap, f->ld, kMixGlobWords};
    const workspace::Want w[] = {want(f->mix.ws, sizeof(double) * wl.doubles()), WANT_STAGED(f->mix.tab, tabBytes), sigmaLocWant(f)};
    return reserveSlots(f, w);
}
// The tables' upload and the arguments of every kernel of a call; P goes to slot `slot` of the scratch image.
int mixPrepare(eqf_filter* f, const MixCall& c, int ref, int dst, int slot, MixArgs& a) {
    const size_t nm = c.members.size(), nu = c.uniq.size();
    const size_t tabBytes = sizeof(MixMember) * nm + sizeof(int) * nu;
    int rc = mixReserve(f, tabBytes);
    if (rc) return rc;
    rc = launchLocal(f, 0, f->B, false);  // (only writes the J records)
    if (rc) return rc;
    f->mix.launches = 1;  // (k_local_jacobian)
    HIPC(f->mix.tab.wait());
    std::memcpy(f->mix.tab.host, c.members.data(), sizeof(MixMember) * nm);
    std::memcpy(f->mix.tab.host + sizeof(MixMember) * nm, c.uniq.data(), sizeof(int) * nu);
    HIPC(f->mix.tab.upload(tabBytes, f->stream));
    const mixture::WorkLayout wl{f->B, f->cap, f->ld, kMixGlobWords};
    double* ws = f->mix.ws;
    a = MixArgs{};
    a.g = f->g[f->pG]; a.p0 = f->p0; a.Q = f->Q[f->pG]; a.cap = f->cap; a.B = f->B;
    a.jac = f->dJac; a.jacT = ws + wl.offJac(); a.est = ws + wl.offEst(); a.err = ws + wl.offErr(); a.mean = ws + wl.offMean();
    a.mem = reinterpret_cast<const MixMember*>(f->mix.tab.dev.get()); a.n = int(nm);
    a.uniq = reinterpret_cast<const int*>(f->mix.tab.dev + sizeof(MixMember) * nm); a.nUniq = int(nu);
    a.N = c.N; a.ref = ref; a.dst = dst;
    a.Sigma = static_cast<double*>(f->Sigma[f->pS]); a.ld = f->ld; a.sigmaStride = f->sigmaStride;
    a.P = f->dSigmaLoc + (long long)slot * f->sigmaStride;
    a.out = ws + wl.offOut(); a.verdict = reinterpret_cast<int*>(ws + wl.offVerdict());
    a.stG = reinterpret_cast<Glob*>(ws + wl.offGlob()); a.stP0 = ws + wl.offP0(); a.stQ = ws + wl.offQ();
    a.lmc = f->lmc;
    a.delta = f->dbgDelta; a.gamma = f->dbgGamma; a.gammaTot = f->dbgGammaTot; a.innov = (f->innovStats && f->dInnov) ? f->dInnov : nullptr;
    HIPC(hipMemsetAsync(a.verdict, 0, sizeof(int) * 4, f->stream));
    return EQF_OK;
}
// errors about the centre, and P: the launches of one pass
void mixPass(eqf_filter* f, const MixArgs& a) {
    const int strips = std::max(1, (a.N + 255) / 256);
    MIX_LAUNCH(f, k_mix_error, dim3(strips, a.nUniq), dim3(256), 0, f->stream, a);
}
void mixReduce(eqf_filter* f, const MixArgs& a) {
    MIX_LAUNCH(f, k_mix_reduce, dim3(mixture::chunks(a.N), mixture::rowBlocks(a.N)), dim3(kMixLanes), 0, f->stream, a);
    MIX_LAUNCH(f, k_mix_report, dim3(1), dim3(256), 0, f->stream, a);
}
void mixFillReport(eqf_mixture_report* r, const MixCall& c, int n, const double* out, int info) {
    const double nan = std::nan("");
    r->n_eff = c.nEff;
    r->spread_trace = info ? nan : out[0];
    r->total_trace = info ? nan : out[1];
    r->n = n;
    r->info = info;
}
}  // namespace

int eqf_get_mixture_moments(eqf_filter* f, int n, const int* idx, const double* w, int ref, int centred, double* mean, double* P, int ld,
    eqf_mixture_report* report) {
    if (!f || !P || (centred != 0 && centred != 1) || !mixture::headArgsOk(n, idx, w, ref, f->B)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    MixCall c;
    int rc = mixCheck(f, n, idx, w, ref, false, c);
    if (rc) return rc;
    const int nr = kBase + 3 * c.N, nn = kLm0 + 3 * c.N;
    if (ld < nr) return EQF_ERR_INVALID;
    MixArgs a;
    rc = mixPrepare(f, c, ref, ref, ref, a);
    if (rc) return rc;
    a.centre = ref; a.centreFilter = ref; a.centred = centred;
    const int strips = std::max(1, (c.N + 255) / 256);
    MIX_LAUNCH(f, k_mix_estimate, dim3(strips, a.nUniq), dim3(256), 0, f->stream, a);
    mixPass(f, a);
    MIX_LAUNCH(f, k_mix_mean, dim3((nn + 255) / 256), dim3(256), 0, f->stream, a);
    mixReduce(f, a);
    hipLaunchKernelGGL(k_sigma_export<double>, dim3((nr + 255) / 256, nr), dim3(256), 0, f->stream, a.P, f->ld, nr, f->dOut, nr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(f->hOut, f->dOut, sizeof(double) * (size_t)nr * nr, hipMemcpyDeviceToHost, f->stream));
    std::vector<double> hm(nn);
    double out[4];
    int verdict[4];
    HIPC(hipMemcpyAsync(hm.data(), a.mean, sizeof(double) * nn, hipMemcpyDeviceToHost, f->stream));
    HIPC(hipMemcpyAsync(out, a.out, sizeof(out), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipMemcpyAsync(verdict, a.verdict, sizeof(verdict), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    const int info = verdict[2];
    const double nan = std::nan("");
    for (int r = 0; r < nr; ++r)
        for (int q = 0; q < nr; ++q) P[(size_t)r * ld + q] = info ? nan : f->hOut[(size_t)r * nr + q];
    if (mean)
        for (int i = 0; i < nr; ++i) mean[i] = info ? nan : hm[mixture::refToPadded(i)];
    if (report) mixFillReport(report, c, n, out, info);
    return EQF_OK;
}

int eqf_merge_filters(eqf_filter* f, int n, const int* idx, const double* w, int ref, int dst, eqf_mixture_report* report) {
    if (!f || dst < 0 || dst >= f->B || !mixture::headArgsOk(n, idx, w, ref, f->B)) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    MixCall c;
    int rc = mixCheck(f, n, idx, w, ref, true, c);
    if (rc) return rc;
    const int nn = kLm0 + 3 * c.N;
    MixArgs a;
    rc = mixPrepare(f, c, ref, dst, dst, a);
    if (rc) return rc;
    const int strips = std::max(1, (c.N + 255) / 256);
    // first pass: eBar about the reference's own estimate; xBar; second pass: the mean-square error about xBar (centred = 0)
    a.centre = ref; a.centreFilter = ref; a.centred = 1;
    MIX_LAUNCH(f, k_mix_estimate, dim3(strips, a.nUniq), dim3(256), 0, f->stream, a);
    mixPass(f, a);
    MIX_LAUNCH(f, k_mix_mean, dim3((nn + 255) / 256), dim3(256), 0, f->stream, a);
    MIX_LAUNCH(f, k_mix_retract, dim3(1), dim3(256), 0, f->stream, a);
    a.centre = f->B; a.centreFilter = -1; a.centred = 0;
    mixPass(f, a);
    mixReduce(f, a);
    // behind the verdict: Sigma, the small state, the constants
    MIX_LAUNCH(f, k_mix_store, dim3((nn + 255) / 256, nn), dim3(256), 0, f->stream, a);
    MIX_LAUNCH(f, k_mix_commit, dim3(std::max(1, (f->cap + 255) / 256)), dim3(256), 0, f->stream, a);
    MIX_LAUNCH(f, k_mix_restore, dim3(std::max(1, (c.N + 127) / 128)), dim3(128), 0, f->stream, a);
    HIPC(hipGetLastError());
    // The host's bookkeeping of dst follows eqf_copy_filters(ref -> dst) -- if the device wrote.  Where that bookkeeping would not change
    // (dst shares the reference's ids, clock and flags and has no gate report: a member, as a rule) the verdict is not waited for.
    const bool same = mirrorsAgree(f, dst, ref);
    int info = 0;
    if (report || !same) {
        double out[4];
        int verdict[4];
        HIPC(hipMemcpyAsync(out, a.out, sizeof(out), hipMemcpyDeviceToHost, f->stream));
        HIPC(hipMemcpyAsync(verdict, a.verdict, sizeof(verdict), hipMemcpyDeviceToHost, f->stream));
        HIPC(hipStreamSynchronize(f->stream));
        info = verdict[2];
        if (report) mixFillReport(report, c, n, out, info);
    }
    if (info == 0) {
        adoptMirror(f, dst, f, ref);  // (dst == ref: only the gate report starts over)
        forgetDeviceCaches(f);
    }
    return EQF_OK;
}

// ---- splitting filters into mixture components (eqf_split.hpp; the host's decisions: eqf_split_host.hpp)
static_assert(split::kRefBase == kBase && split::kPadBase == kLm0 && split::kOk == EQF_OK && split::kInvalid == EQF_ERR_INVALID &&
                  sizeof(split::Source) == sizeof(SplitSource) && sizeof(split::Child) == sizeof(SplitChild) &&
                  sizeof(split::Pair) == sizeof(ClonePair) && offsetof(split::Pair, N) == offsetof(ClonePair, N) &&
                  split::kAxisRows == kSplitAxisRows && split::kTileRows == kSplitTileRows && split::kTileCols == kSplitTileCols,
    "eqf_split_host.hpp repeats the layout constants, the tables and the error codes");

int eqf_split_filters(eqf_filter* f, int local, const double* a, int lda, int n, const int* dst_idx, const int* src_idx, const double* shift,
    const double* shrink, double* gamma, int ldg, eqf_split_report* report) {
    if (!f) return EQF_ERR_INVALID;
    int rc = split::headCheck(f->B, local, a, n, dst_idx, src_idx, shift, shrink);
    if (rc) return rc;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    if (n == 0) return EQF_OK;
    GATE(f);  // (queued IMU calls and a pending gate first: the gate may still change the landmark counts)
    const int B = f->B;
    const std::vector<int> N = landmarkCounts(f);
    rc = split::rowCheck(a, lda, n, src_idx, gamma ? ldg : -1, N.data());
    if (rc) return rc;
    split::Plan pl;
    split::group(B, n, dst_idx, src_idx, N.data(), pl);
    const split::Image im{size_t(B), size_t(f->cap)};
    const split::Work wk{size_t(B), size_t(f->ld)};
    {
        const workspace::Want w[] = {WANT_STAGED(f->split.img, im.bytes()), want(f->split.ws, wk.bytes())};
        rc = reserveSlots(f, w);
        if (rc) return rc;
    }
    if (local) {
        rc = launchLocal(f, 0, B, false);  // (only writes the J records)
        if (rc) return rc;
    }
    HIPC(f->split.img.wait());
    split::fillImage(im, pl, a, lda, shift, shrink, f->split.img.host);
    HIPC(f->split.img.upload(im.bytes(), f->stream));
    const int ns = int(pl.sources.size()), np = int(pl.pairs.size());
    char* di = f->split.img.dev;
    double* ws = reinterpret_cast<double*>(f->split.ws.get());
    SplitArgs sa{};
    sa.Sigma = static_cast<const double*>(f->Sigma[f->pS]); sa.SigmaW = static_cast<double*>(f->Sigma[f->pS]); sa.ld = f->ld;
    sa.sigmaStride = f->sigmaStride;
    sa.rows = reinterpret_cast<const double*>(di + im.offRows()); sa.ldr = int(im.ldr());
    sa.shift = reinterpret_cast<const double*>(di + im.offShift()); sa.shrink = reinterpret_cast<const double*>(di + im.offShrink());
    sa.sources = reinterpret_cast<const SplitSource*>(di + im.offSources()); sa.ns = ns;
    sa.children = reinterpret_cast<const SplitChild*>(di + im.offChildren());
    sa.pairs = reinterpret_cast<ClonePair*>(di + im.offPairs());
    sa.jac = local ? f->dJac.get() : nullptr; sa.cap = f->cap;
    sa.Ht = ws + wk.offHt(); sa.Bv = ws + wk.offB(); sa.U = ws + wk.offU(); sa.G = ws + wk.offG(); sa.rec = ws + wk.offRec();
    sa.mask = reinterpret_cast<unsigned char*>(ws + wk.offMask());
    hipStream_t st = f->stream;
    HIPC(hipMemsetAsync(sa.mask, 0, size_t(B), st));  // (filters that are no child's dst are not moved)
    hipLaunchKernelGGL(k_split_row, dim3(ns), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_split_axis, dim3(split::axisBlocks(pl.maxN), ns), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_split_verdict, dim3(ns), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_split_sigma, dim3(split::tileColBlocks(pl.maxN), split::tileRowBlocks(pl.maxN), std::min(ns, 65535)), dim3(256), 0, st, sa);
    // everything that is not Sigma: the clone route's kernels over the pairs the verdicts have left, then the plain group step
    if (np > 0) {
        CloneSmallArgs ma{};
        ma.src = cloneSide(f); ma.dst = cloneSide(f); ma.restore = 1;
        ma.pairs = sa.pairs; ma.nPairs = np;
        hipLaunchKernelGGL(k_clone_small, dim3(std::max(1, (f->cap + 255) / 256), std::min(np, 65535)), dim3(256), 0, st, ma);
        hipLaunchKernelGGL(k_clone_restore, dim3(std::max(1, (pl.maxN + 127) / 128), std::min(np, 65535)), dim3(128), 0, st, f->g[f->pG].get(),
            f->p0.get(), f->lmc.get(), f->cap, f->errflag.get(), sa.pairs, np);
    }
    IncArgs ia{};
    ia.g = f->g[f->pG]; ia.p0 = f->p0; ia.Q = f->Q[f->pG]; ia.cap = f->cap; ia.gamma = sa.G; ia.strideG = f->ld; ia.off = 0; ia.mask = sa.mask;
    hipLaunchKernelGGL(k_apply_increment, dim3(B), dim3(256), 0, st, ia);  // (always the plain lift: ia.lift stays NULL)
    HIPC(hipGetLastError());
    forgetDeviceCaches(f);  // (as behind eqf_copy_filters)
    // The host's bookkeeping of a dst follows eqf_copy_filters(src -> dst) -- if the device wrote.  Where no dst's bookkeeping would change
    // (eqf_merge_filters' rule) the verdicts are not waited for.
    bool same = true;
    for (const auto& c : pl.children) {
        const int d = c.dst, s = pl.sources[c.source].src;
        if (d != s && !mirrorsAgree(f, d, s)) same = false;
    }
    if (!gamma && !report && same) return EQF_OK;
    std::vector<double> hRec(size_t(2) * ns), hG;
    HIPC(hipMemcpyAsync(hRec.data(), sa.rec, sizeof(double) * hRec.size(), hipMemcpyDeviceToHost, st));
    if (gamma) {
        hG.resize(size_t(B) * f->ld);
        HIPC(hipMemcpyAsync(hG.data(), sa.G, sizeof(double) * hG.size(), hipMemcpyDeviceToHost, st));
    }
    HIPC(hipStreamSynchronize(st));
    // (read first: the mirrors of the sources are not among the destinations that change, by the dst/src rule)
    for (const auto& c : pl.children) {
        const int d = c.dst, s = pl.sources[c.source].src, info = int(hRec[size_t(2) * c.source + 1]);
        if (report) {
            report[c.call].S = hRec[size_t(2) * c.source];
            report[c.call].info = info;
        }
        if (gamma) linear::unpackGamma(hG.data() + size_t(d) * f->ld, N[s], gamma + size_t(c.call) * ldg, info != 0);
        if (info == 0 && d != s) adoptMirror(f, d, f, s);
    }
    return EQF_OK;
}

// ---- pairwise merge costs (eqf_mergecost.hpp; argument checks, items, chunk plan and cost formulas: eqf_mergecost_host.hpp)
static_assert(mergecost::kRefBase == kBase && mergecost::kPadBase == kLm0 && mergecost::kBlock == kSB &&
              sizeof(mergecost::Item) == sizeof(PairItem) && mergecost::kRec == kPairRec && sizeof(Glob) % 8 == 0,
    "eqf_mergecost_host.hpp repeats the layout constants");
namespace {
mergecost::WorkLayout mcWork(const eqf_filter* f, int C) {
    return {size_t(C), size_t(f->sigmaStride), size_t(f->nTot), size_t(kDRec), size_t(kNeesHead + kNeesRhs), sizeof(Glob) / 8};
}
// both blocks of a call; a block this call installed is zero-filled where its unused parts are read
int mcReserve(eqf_filter* f, int chunk, size_t nItems) {
    const size_t wsBytes = sizeof(double) * mcWork(f, chunk).doubles();
    const workspace::Want w[] = {want(f->mc.ws, wsBytes, &f->mc.wsBytes),
        want(f->mc.items, mergecost::ItemsLayout{nItems}.bytes(), &f->mc.itemBytes)};
    workspace::Result got;
    const int rc = reserveSlots(f, w, &got);
    if (rc) return rc;
    if (got.has(0)) {
        f->mc.chunkCap = chunk;
        HIPC(hipMemsetAsync(f->mc.ws, 0, wsBytes, f->stream));  // (upper triangles and the Globs are read, never used)
    }
    if (got.has(1)) f->mc.itemCap = nItems;
    return EQF_OK;
}
}  // namespace

int eqf_get_merge_costs(eqf_filter* f, int n, const int* idx, const double* w, int ref, int kind, int first, int npairs, const int* pairs,
    eqf_pair_cost* out, eqf_sigma_stats* member) {
    if (!f || !mixture::headArgsOk(n, idx, w, ref, f->B) || !mergecost::pairArgsOk(n, kind, first, npairs, pairs) || (npairs > 0 && !out))
        return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    MixCall c;
    int rc = mixCheck(f, n, idx, w, ref, false, c);
    if (rc) return rc;
    mergecost::distinct(n, idx, f->B, c.uniq);  // (every member's image is needed, a member of weight 0 too)
    std::vector<mergecost::Item> items;
    mergecost::buildItems(n, idx, c.wt.data(), kind, npairs, pairs, items);
    const int chunk = mergecost::chunkSize(f->mc.chunkOpt, f->B);
    rc = mcReserve(f, chunk, items.size());
    if (rc) return rc;
    // e_b, J'_b and Sigma'_b of every distinct member about c = xHat_ref
    const int launchesBefore = f->mix.launches;  // (eqf_debug_mixture_launches keeps answering for the most recent MIXTURE call)
    MixArgs a;
    rc = mixPrepare(f, c, ref, ref, ref, a);
    f->mix.launches = launchesBefore;
    if (rc) return rc;
    a.centre = ref; a.centreFilter = ref; a.centred = 0;
    const int N = c.N, strips = std::max(1, (N + 255) / 256);
    hipLaunchKernelGGL(k_mix_estimate, dim3(strips, a.nUniq), dim3(256), 0, f->stream, a);
    hipLaunchKernelGGL(k_mix_error, dim3(strips, a.nUniq), dim3(256), 0, f->stream, a);
    for (int u : c.uniq) {
        LocalArgs la = localArgs(f, u);
        la.jac = a.jacT;
        hipLaunchKernelGGL(k_sigma_local, dim3(strips, std::max(1, (N + kLocalRows - 1) / kLocalRows), 1), dim3(256), 0, f->stream, la);
    }
    HIPC(hipGetLastError());
    const int off = mergecost::offsetOf(first), m = mergecost::paddedOrder(N, off);
    const mergecost::WorkLayout wl = mcWork(f, f->mc.chunkCap);
    const mergecost::ItemsLayout il{f->mc.itemCap};
    double* ws = reinterpret_cast<double*>(f->mc.ws.get());
    double *wsW = ws + wl.offW(), *wsE = ws + wl.offE(), *wsD = ws + wl.offD(), *wsOut = ws + wl.offOut();
    Glob* wsG = reinterpret_cast<Glob*>(ws + wl.offGlob());
    PairItem* dItems = reinterpret_cast<PairItem*>(f->mc.items + il.offItems());
    double* dRec = reinterpret_cast<double*>(f->mc.items + il.offRecords());
    HIPC(hipMemcpyAsync(dItems, items.data(), sizeof(PairItem) * items.size(), hipMemcpyHostToDevice, f->stream));
    PairArgs pa{};
    pa.items = dItems; pa.S = f->dSigmaLoc; pa.ld = f->ld; pa.strideS = f->sigmaStride; pa.err = a.err; pa.jacT = a.jacT; pa.cap = f->cap;
    pa.N = N; pa.off = off; pa.kind = kind; pa.W = wsW; pa.E = wsE; pa.ldE = std::max(m, 1); pa.wg = wsG; pa.neesOut = wsOut; pa.rec = dRec;
    NeesArgs na{};
    na.g = wsG; na.A = wsW; na.ld = f->ld; na.strideA = f->sigmaStride; na.E = wsE; na.ldE = pa.ldE; na.D = wsD;
    na.bad = reinterpret_cast<int*>(ws + wl.offBad());
    na.jac = nullptr; na.cap = f->cap; na.off = off; na.nrhs = 1; na.out = wsOut;
    // the members, then the pairs: chunks of at most `chunk` images, never both kinds in one
    const long long seg0[2] = {0, n}, segLen[2] = {n, npairs};
    for (int s = 0; s < 2; ++s)
        for (int ch = 0; ch < mergecost::numChunks(segLen[s], chunk); ++ch) {
            const int cnt = mergecost::chunkCount(segLen[s], chunk, ch);
            pa.item0 = int(seg0[s] + (long long)ch * chunk);
            pa.count = cnt;
            hipLaunchKernelGGL(k_pair_form, dim3(kLm0 + 3 * N + 1, cnt), dim3(256), 0, f->stream, pa);
            rc = enqueueFactor(f->stream, f->nees.ldsSet, na, cnt, m, 1);
            if (rc) return rc;
            hipLaunchKernelGGL(k_nees_tail, dim3(cnt), dim3(256), 0, f->stream, na);
            hipLaunchKernelGGL(k_pair_tail, dim3((cnt + 255) / 256), dim3(256), 0, f->stream, pa);
        }
    HIPC(hipGetLastError());
    std::vector<double> hR(items.size() * kPairRec);
    HIPC(hipMemcpyAsync(hR.data(), dRec, sizeof(double) * hR.size(), hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    if (member)
        for (int k = 0; k < n; ++k) {
            const double* r = hR.data() + size_t(k) * kPairRec;
            member[k].logdet = r[1];
            member[k].min_pivot = r[4];
            member[k].dof = int(r[5]);
            member[k].info = int(r[3]);
        }
    for (int p = 0; p < npairs; ++p) {
        const double* r = hR.data() + (size_t(n) + p) * kPairRec;
        out[p].cost = r[0];
        out[p].logdet_pair = r[1];
        out[p].maha = r[2];
        out[p].info = int(r[3]);
        out[p].pad_ = 0;
    }
    return EQF_OK;
}

// ---- scoring candidate frames (eqf_score.hpp; argument checks, id matching, chunk plan and record arithmetic: eqf_score_host.hpp)
static_assert(score::kBlock == kSB && sizeof(score::Item) == sizeof(ScoreItem) && score::kOk == EQF_OK && score::kInvalid == EQF_ERR_INVALID &&
              score::kCapacity == EQF_ERR_CAPACITY && score::kUnsorted == EQF_ERR_UNSORTED,
    "eqf_score_host.hpp repeats the layout constants and the error codes");
namespace {
score::WorkLayout scWork(const eqf_filter* f, int C) { return {size_t(C), size_t(score::paddedOrder(f->cap)), size_t(kDRec)}; }
// both blocks of a call; a workspace this call installed is zero-filled
int scReserve(eqf_filter* f, int chunk, size_t tabBytes) {
    const size_t wsBytes = sizeof(double) * scWork(f, chunk).doubles();
    const workspace::Want w[] = {want(f->sc.ws, wsBytes, &f->sc.wsBytes), want(f->sc.tab, tabBytes, &f->sc.tabBytes)};
    workspace::Result got;
    const int rc = reserveSlots(f, w, &got);
    if (rc) return rc;
    if (got.has(0)) {
        f->sc.chunkCap = chunk;
        HIPC(hipMemsetAsync(f->sc.ws, 0, wsBytes, f->stream));  // (upper triangles of diagonal tiles are read, never used)
    }
    return EQF_OK;
}
}  // namespace

int eqf_score_vision(eqf_filter* f, int ncand, const int* nb, const int* ids, const double* bearings, int stride, const unsigned char* mask,
    eqf_frame_score* out, double* nis_lm, unsigned char* used) {
    if (!f || !nb || !ids || !bearings || !out || ncand < 1 || stride < 1) return EQF_ERR_INVALID;
    const int B = f->B, cap = f->cap;
    {
        const int rc = score::checkArgs(B, cap, ncand, nb, ids, bearings, stride, mask);
        if (rc) return rc;
    }
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    // the items: per candidate the matched slots in the state's order, the bearings permuted into it
    const size_t nItems = size_t(B) * ncand;
    std::vector<score::Item> items(nItems);
    std::vector<int> slots, pos;
    int mLm = 0;
    for (int b = 0; b < B; ++b) {
        const bool masked = mask && !mask[b];
        const bool live = !masked && f->init[b];
        for (int c = 0; c < ncand; ++c) {
            const size_t it = size_t(b) * ncand + c;
            const int first = int(slots.size());
            const int m = live ? score::matchItem(int(f->ids[b].size()), f->ids[b].data(), nb[it], ids + it * stride, slots, pos) : 0;
            items[it] = score::Item{b, m, first, masked ? 1 : 0};
            mLm = std::max(mLm, m);
        }
    }
    const size_t nMatched = slots.size();
    std::vector<double> y(3 * nMatched);
    for (size_t it = 0; it < nItems; ++it)
        for (int k = 0; k < items[it].m; ++k)
            std::memcpy(&y[3 * (size_t(items[it].first) + k)], bearings + (it * stride + size_t(pos[size_t(items[it].first) + k])) * 3, sizeof(double) * 3);
    std::vector<double> hRec(nItems * score::kRec, 0.0), hLm(nMatched, 0.0);
    if (nMatched > 0) {
        const int chunk = score::chunkSize(f->sc.chunkOpt, B);
        const score::TabLayout tab{nItems, nMatched};
        int rc = scReserve(f, chunk, tab.bytes());
        if (rc) return rc;
        const score::WorkLayout wl = scWork(f, f->sc.chunkCap);
        double* ws = reinterpret_cast<double*>(f->sc.ws.get());
        ScoreArgs a{};
        a.items = reinterpret_cast<const ScoreItem*>(f->sc.tab + tab.offItems());
        a.slots = reinterpret_cast<const int*>(f->sc.tab + tab.offSlots());
        a.y = reinterpret_cast<const double*>(f->sc.tab + tab.offY());
        a.nisLm = reinterpret_cast<double*>(f->sc.tab + tab.offNisLm());
        a.rec = reinterpret_cast<double*>(f->sc.tab + tab.offRec());
        a.Q = f->Q[f->pG]; a.lmc = f->lmc; a.S = static_cast<const double*>(f->Sigma[f->pS]); a.sigmaStride = f->sigmaStride; a.ld = f->ld;
        a.cap = cap; a.measVar = f->set.measurementVariance;
        a.ldW = score::paddedOrder(cap); a.strideW = (long long)a.ldW * a.ldW; a.W = ws + wl.offW(); a.E = ws + wl.offE(); a.D = ws + wl.offD();
        a.bad = reinterpret_cast<int*>(ws + wl.offBad());
        HIPC(hipMemcpyAsync(f->sc.tab + tab.offItems(), items.data(), sizeof(ScoreItem) * nItems, hipMemcpyHostToDevice, f->stream));
        HIPC(hipMemcpyAsync(f->sc.tab + tab.offSlots(), slots.data(), sizeof(int) * nMatched, hipMemcpyHostToDevice, f->stream));
        HIPC(hipMemcpyAsync(f->sc.tab + tab.offY(), y.data(), sizeof(double) * 3 * nMatched, hipMemcpyHostToDevice, f->stream));
        for (int ch = 0; ch < score::numChunks((long long)nItems, chunk); ++ch) {
            const int cnt = score::chunkCount((long long)nItems, chunk, ch);
            a.item0 = ch * chunk;
            a.count = cnt;
            hipLaunchKernelGGL(k_score_form, dim3((mLm + 3) / 4 + 1, cnt), dim3(256), 0, f->stream, a);
            rc = enqueueFactor(f->stream, f->sc.ldsSet, a, cnt, 2 * mLm, 1);
            if (rc) return rc;
            hipLaunchKernelGGL(k_score_tail, dim3(cnt), dim3(256), 0, f->stream, a);
        }
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(hRec.data(), f->sc.tab + tab.offRec(), sizeof(double) * hRec.size(), hipMemcpyDeviceToHost, f->stream));
        HIPC(hipMemcpyAsync(hLm.data(), f->sc.tab + tab.offNisLm(), sizeof(double) * nMatched, hipMemcpyDeviceToHost, f->stream));
    }
    HIPC(hipStreamSynchronize(f->stream));
    if (nis_lm) std::fill(nis_lm, nis_lm + nItems * stride, 0.0);
    if (used) std::fill(used, used + nItems * stride, (unsigned char)0);
    const double nan = std::nan("");
    for (size_t it = 0; it < nItems; ++it) {
        const score::Item& im = items[it];
        eqf_frame_score& o = out[it];
        if (im.masked) {
            o.nis = o.logdet_S = o.loglik = nan;
            o.dof = 0;
            o.info = score::kInfoMasked;
            continue;
        }
        const double* r = hRec.data() + it * score::kRec;  // (all zero where nothing matched anywhere in the call)
        o.nis = r[0];
        o.logdet_S = r[1];
        o.loglik = r[2];
        o.dof = int(r[3]);
        o.info = int(r[4]);
        for (int k = 0; k < im.m; ++k) {
            const size_t e = it * stride + size_t(pos[size_t(im.first) + k]);
            if (nis_lm) nis_lm[e] = hLm[size_t(im.first) + k];
            if (used) used[e] = 1;
        }
    }
    return EQF_OK;
}

int eqf_debug_mixture_launches(eqf_filter* f) { return f ? f->mix.launches : EQF_ERR_INVALID; }
int eqf_debug_iterate_launches(eqf_filter* f) { return f ? f->iter.launches : EQF_ERR_INVALID; }

int eqf_debug_sigma_pad(eqf_filter* f, int b, int image, double* max_abs) {
    if (!f || b < 0 || b >= f->B || (image != 0 && image != 1) || !max_abs) return EQF_ERR_INVALID;
    if (f->precision != EQF_PRECISION_F64) return EQF_ERR_UNSUPPORTED;
    GATE(f);
    if (image == 1 && !f->dSigmaLoc) return EQF_ERR_INVALID;
    const double* S = (image ? f->dSigmaLoc : static_cast<const double*>(f->Sigma[f->pS])) + (long long)b * f->sigmaStride;
    const int nn = kLm0 + 3 * int(f->ids[b].size());
    std::vector<double> row(nn), col(nn);
    HIPC(hipStreamSynchronize(f->stream));
    HIPC(hipMemcpy(row.data(), S + (long long)kBase * f->ld, sizeof(double) * nn, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy2D(col.data(), sizeof(double), S + kBase, sizeof(double) * f->ld, sizeof(double), nn, hipMemcpyDeviceToHost));
    double m = 0.0;
    for (int i = 0; i < nn; ++i) {  // (a NaN counts as not zero)
        const double r = std::fabs(row[i]), c = std::fabs(col[i]);
        m = (r > m || r != r) ? r : m;
        m = (c > m || c != c) ? c : m;
        if (m != m) break;
    }
    *max_abs = m;
    return EQF_OK;
}

int eqf_tile_syrk_i8(int device, void* stream, int batch, const int* nv, const int* mp, const double* Y, int ldY, long long strideY,
    const double* Sin, double* Sout, int ld, long long sigmaStride, int slices, void* workspace, size_t workspace_bytes) {
    if (batch < 1 || !nv || !mp || !Y || !Sin || !Sout || !workspace || slices < 5 || slices > 7 || Sin == Sout) return EQF_ERR_INVALID;
    int nvMax = 1, mpMax = 32;
    for (int b = 0; b < batch; ++b) {
        if (nv[b] < 1 || mp[b] < 0 || mp[b] % 32 || nv[b] > ld || nv[b] > ldY) return EQF_ERR_INVALID;
        nvMax = std::max(nvMax, nv[b]);
        mpMax = std::max(mpMax, mp[b]);
    }
    if (!i8Exact(mpMax, slices)) return EQF_ERR_INVALID;
    if ((long long)ld * nvMax > sigmaStride && batch > 1) return EQF_ERR_INVALID;
    if ((long long)ldY * mpMax > strideY && batch > 1) return EQF_ERR_INVALID;
    if (workspace_bytes < eqf_tile_syrk_i8_workspace_bytes(batch, nvMax, mpMax, slices)) return EQF_ERR_INVALID;
    DeviceScope ds(device);
    if (!ds.ok) return EQF_ERR_HIP;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // layout of the workspace: the dims [batch][2], the exponent words, the slices (1 KB aligned)
    const long long stride = i8SliceBytes(mpMax, nvMax, slices);
    const int expoWords = i8ddExpoWords(nvMax);
    char* ws = static_cast<char*>(workspace);
    int* dDims = reinterpret_cast<int*>(ws);
    int* dExpo = dDims + roundUp(2 * batch, 256);
    signed char* dSl = reinterpret_cast<signed char*>(ws + roundUp(int(sizeof(int)) * (roundUp(2 * batch, 256) + expoWords * batch), 1024));
    std::vector<int> hd(2 * batch);
    for (int b = 0; b < batch; ++b) {
        hd[2 * b] = nv[b];
        hd[2 * b + 1] = mp[b];
    }
    HIPC(hipStreamSynchronize(st));  // (the workspace may still be in use by an earlier call on this stream)
    HIPC(hipMemcpy(dDims, hd.data(), sizeof(int) * 2 * batch, hipMemcpyHostToDevice));
    I8DdArgs ia{};
    ia.Y = Y; ia.ldY = ldY; ia.strideY = strideY;
    ia.Sin = Sin; ia.Sout = Sout; ia.ld = ld; ia.sigmaStride = sigmaStride;
    ia.g = nullptr; ia.dims = dDims; ia.pad = 32; ia.skipCol = -1;
    ia.ws = dSl; ia.wsStride = stride; ia.expo = dExpo; ia.expoStride = expoWords;
    ia.B = batch; ia.nt = (nvMax + 63) / 64;
    launchI8Dd(slices, ia, nullptr, (nvMax + 31) / 32, st);
    HIPC(hipGetLastError());
    return EQF_OK;
}

size_t eqf_tile_syrk_i8_workspace_bytes(int batch, int max_nv, int max_mp, int slices) {
    if (batch < 1 || max_nv < 1 || max_mp < 0 || slices < 5 || slices > 7) return 0;
    max_mp = std::max(roundUp(max_mp, 32), 32);
    const long long head = roundUp(int(sizeof(int)) * (roundUp(2 * batch, 256) + i8ddExpoWords(max_nv) * batch), 1024);
    return size_t(head + i8SliceBytes(max_mp, max_nv, slices) * batch);
}

int eqf_set_imu_burst(eqf_filter* f, int max_steps) {
    if (!f || max_steps < 0) return EQF_ERR_INVALID;
    GATE(f);
    f->burstMax = std::min(max_steps, kBurstMax);
    return EQF_OK;
}

int eqf_set_dense_propagate(eqf_filter* f, int on) {
    if (!f) return EQF_ERR_INVALID;
    GATE(f);
    HIPC(hipSetDevice(f->device));
    if (on && !f->dF) {
        const size_t bytes = f->esz * f->sigmaStride * f->B;
        const workspace::Want w[] = {want(f->dF, bytes), want(f->dG, bytes), want(f->dBn, f->esz * (size_t)f->nTot * 6 * f->B)};
        const int rc = reserveSlots(f, w);
        if (rc) return rc;
        HIPC(hipMemset(f->dF, 0, bytes));
        HIPC(hipMemset(f->dG, 0, bytes));
    }
    f->densePropagate = on ? 1 : 0;
    f->csValid = false;
    return EQF_OK;
}

int eqf_profile_enable(eqf_filter* f, int on) {
    if (!f) return EQF_ERR_INVALID;
    GATE(f);
    if (f->prof && !on) {
        int rc = profDrain(f);
        if (rc) return rc;
    }
    f->prof = on != 0;
    if (on) {
        // calibrate the bracket itself: two event records with nothing in between still measure a few microseconds,
        // which would otherwise be charged to every kernel
        std::fill(std::begin(f->profCount), std::end(f->profCount), 0);
        std::fill(std::begin(f->profMs), std::end(f->profMs), 0.0);
        for (auto& v : f->profSamples) v.clear();
        f->profOverheadMs = 0.0;
        // (median of 64 empty brackets: a single hiccup must not be charged to every kernel)
        for (int i = 0; i < 64; ++i) {
            int rc = profiled(f, EQF_PROF_CHURN, [] {});
            if (rc) return rc;
        }
        HIPC(hipStreamSynchronize(f->stream));
        std::vector<float> el;
        for (auto& p : f->profPairs) {
            float ms = 0;
            HIPC(hipEventElapsedTime(&ms, p.a, p.b));
            el.push_back(ms);
            f->evPool.push_back(p.a);
            f->evPool.push_back(p.b);
        }
        f->profPairs.clear();
        std::sort(el.begin(), el.end());
        f->profOverheadMs = el.empty() ? 0.0 : el[el.size() / 2];
    }
    return EQF_OK;
}

int eqf_profile_get(eqf_filter* f, int cls, long long* launches, double* total_ms) {
    if (!f || cls < 0 || cls >= EQF_PROF_CLASSES) return EQF_ERR_INVALID;
    GATE(f);
    int rc = profDrain(f);
    if (rc) return rc;
    if (launches) *launches = f->profCount[cls];
    if (total_ms) {
        // An event bracket measures kernel time PLUS whatever the stream waited for the host between the two records (the
        // profiled pass triples the API calls per launch, so a small problem is host-bound in it: brackets of one and the
        // same launch then read 13 us or 40 us by chance).  Launches of one class and one shape key do identical work, so
        // each shape is charged its MEDIAN bracket times its launch count; different shapes (chain step 0 vs step 9, the
        // launch that carries the downdate) are never compared with each other.
        std::vector<ProfSample> v = f->profSamples[cls];
        std::sort(v.begin(), v.end(), [](const ProfSample& x, const ProfSample& y) { return x.key != y.key ? x.key < y.key : x.ms < y.ms; });
        double sum = 0.0;
        for (size_t i = 0; i < v.size();) {
            size_t j = i;
            while (j < v.size() && v[j].key == v[i].key) ++j;
            sum += double(v[i + (j - i) / 2].ms) * double(j - i);
            i = j;
        }
        *total_ms = std::max(0.0, sum - f->profOverheadMs * f->profCount[cls]);
    }
    return EQF_OK;
}

const char* eqf_profile_class_name(int cls) {
    static const char* names[EQF_PROF_CLASSES] = {"k_propagate", "k_update_prep", "k_chol_step", "k_update_reduce", "k_update_finish",
        "k_downdate", "churn", "k_dense_riccati", "k_imu_burst", "k_chol_step_dd", "k_chol_resident", "k_lin_rows", "k_lin_gain",
        "k_lin_solve", "k_lin_downdate"};
    return (cls >= 0 && cls < EQF_PROF_CLASSES) ? names[cls] : "?";
}

}  // extern "C"
