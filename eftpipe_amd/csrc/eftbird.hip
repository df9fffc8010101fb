// eftbird.hip -- C ABI of libeftbird.so (see include/eftbird.h) and the stage scheduler.
// gfx950 only.  No CPU fallback: every entry point needs a HIP device.
#include "../../include/eftbird.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <tuple>
#include <algorithm>
#include <vector>

#include "eftb_kernels.hpp"
#include "eftb_own.hpp"
#include "eftb_staged.hpp"

using namespace eftb;

constexpr size_t GEMM_LDS = (size_t)64 * 258 * sizeof(double);  // A tile of gemm_rows_kernel

// What-if builds only (make whatif -> libeftbird_whatif.so, tools/whatif_probe.py): EFTB_WHATIF_SKIP is a set of direct-P_l kernels that are NOT
// launched, to see what each one costs the pipelined step (the results of such a run are garbage).  The product library has no such switch.
#ifdef EFTB_WHATIF
static const int g_whatif = getenv("EFTB_WHATIF_SKIP") ? atoi(getenv("EFTB_WHATIF_SKIP")) : 0;
#define WHATIF_SKIP(bit) ((g_whatif & (bit)) != 0)
#else
#define WHATIF_SKIP(bit) false
#endif

static thread_local std::string g_err;

static int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

// (a failed call's error is reported here: the runtime would otherwise keep it for the next hipGetLastError, some other call's launch check)
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            (void)hipGetLastError();                                                          \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                     \
    } while (0)

// Everything that is acquired -- device memory (zero: filled with zeros on the null stream), page-locked memory, events (flags 0: a timing
// event), streams -- is acquired here and held by a ledger (eftb_own.hpp) from then on: the engine's, or a probe's local one.  The ledger
// alone releases; the pointers the callers keep only view.  (eftb_host_alloc / eftb_host_free: the caller's memory, not held anywhere.)
static void drop_dev(void* p) { (void)hipFree(p); }
static void drop_host(void* p) { (void)hipHostFree(p); }
static void drop_event(void* p) { (void)hipEventDestroy(static_cast<hipEvent_t>(p)); }
static void drop_stream(void* p) { (void)hipStreamDestroy(static_cast<hipStream_t>(p)); }

template <class T>
static hipError_t own_dev(Ledger& own, T** p, size_t bytes, bool zero = false) {
    void* q = nullptr;
    *p = nullptr;
    if (hipError_t st = hipMalloc(&q, bytes); st != hipSuccess) return st;
    own.hold(q, drop_dev);
    *p = static_cast<T*>(q);
    return zero ? hipMemset(q, 0, bytes) : hipSuccess;
}

template <class T>
static hipError_t own_host(Ledger& own, T** p, size_t bytes, unsigned flags) {
    void* q = nullptr;
    *p = nullptr;
    if (hipError_t st = hipHostMalloc(&q, bytes, flags); st != hipSuccess) return st;
    own.hold(q, drop_host);
    *p = static_cast<T*>(q);
    return hipSuccess;
}

static hipError_t own_event(Ledger& own, hipEvent_t* ev, unsigned flags = 0) {
    *ev = nullptr;
    if (hipError_t st = flags ? hipEventCreateWithFlags(ev, flags) : hipEventCreate(ev); st != hipSuccess) return st;
    own.hold(*ev, drop_event);
    return hipSuccess;
}

static hipError_t own_stream(Ledger& own, hipStream_t* s, int prio) {
    *s = nullptr;
    if (hipError_t st = hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio); st != hipSuccess) return st;
    own.hold(*s, drop_stream);
    return hipSuccess;
}

struct eftb_engine {
    eftb_config c;
    Ledger own;  // everything below that came from the device runtime; released newest first when the engine is deleted (eftb_destroy)
    hipStream_t stream = nullptr, side = nullptr;   // side: the small input-only kernels (IR filters, AP prefix sums) run beside the loop path
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evFork = nullptr, evJoin = nullptr, evJoinAP = nullptr;  // evJoin: X, Y, Q(f) ready; evJoinAP: AP prefix sums + knot weights ready
    bool finalized = false;
    void* tab[EFTB_T_COUNT] = {nullptr};
    size_t tab_bytes[EFTB_T_COUNT] = {0};
    double* buf[EFTB_B_COUNT] = {nullptr};
    size_t buf_elems[EFTB_B_COUNT] = {0};
    // scratch
    double *SD = nullptr, *Talt = nullptr, *part = nullptr;
    double *RSA = nullptr, *RSC = nullptr;  // matrix-core resum: A = Q V8^T [B][80][8] (Nl = 2), per-s records [B][NS][48]
    double *RSAS = nullptr, *RSAS2 = nullptr;  // Nl = 3: the A operand per s [B][NS][4][64][2] (resum_as_kernel: inputs only), two sets like RSA / RSC
    hipEvent_t evXY = nullptr, evAS = nullptr;  // X, Y of this run are in place (look-ahead stream); the per-s operand built beside the chain is ready
    double *RSA2 = nullptr, *RSC2 = nullptr;  // second operand set: the look-ahead builds run i+1's operands while run i's resummation reads its own
    hipEvent_t evRsDone[2] = {nullptr, nullptr};  // the resummation that read operand set [slot] has finished
    unsigned rs_step = 0;
    // flow control of asynchronous runs: at most RUN_DEPTH runs are in flight (a caller that never synchronises cannot grow the runtime's
    // command queues without bound; four runs ahead is more than the three-stream layout can use)
    static constexpr int RUN_DEPTH = 8;
    hipEvent_t evRun[RUN_DEPTH] = {};
    unsigned long long run_seq = 0;
    bool nnlo_inline = true;  // EFTB_NNLO_INLINE=0: with_NNLO steps never take the three-stream layout
    // duration of the dominant kernel inside pipelined steps (EFTB_O_TIME_DOMINANT): HIP events on the stream it is launched on
    static constexpr int NTIMER = 8;
    hipEvent_t evT0[NTIMER] = {}, evT1[NTIMER] = {};
    bool timer_busy[NTIMER] = {};
    unsigned timer_next = 0;
    int time_dominant = 0;          // 0 off; n: every n-th launch of the timed kernel is bracketed
    int time_kernel = 1;            // EFTB_O_TIME_KERNEL, bits: 1 the resummation kernel, 2 the synthesis launch of the loop stages, 4 the AP kernel (knot weights; direct-P_l runs: ap_plk_kernel)
    unsigned long long time_seqk[3] = {};
    int timer_kind[NTIMER] = {};    // which kernel the pair of a slot brackets (see time_kernel)
    double timer_ms[3] = {};
    long long timer_n[3] = {};
    long long timer_cosmo[3] = {};   // cosmologies the timed launches carried (a launch of coalesced steps carries several steps' worth)
    int timer_B[8] = {};             // batch of the launch slot t brackets (NTIMER = 8)
    int launch_B = 0;                // batch of the launch being issued (launch_stages_impl)
    double *APP = nullptr, *APR = nullptr, *APP2 = nullptr, *APR2 = nullptr;  // AP: prefix sums over mu [B][nmu+1][Nl*Nl*4], roots [B][nmu]
    // AP fast path (ap_weights_kernel / ap_rows_kernel): knot weights [B][tiles][APW_DCAP][Nl][Nl][2][64], lowest knot per k [B][tiles * 64],
    // window per tile [B][tiles]; second set for the look-ahead of overlapped runs (swapped together with APP / APR)
    double *APW = nullptr, *APW2 = nullptr;
    int *API = nullptr, *API2 = nullptr;
    int4 *APM = nullptr, *APM2 = nullptr;
    // EFTB_AP_MODE: 0 = knot weights + banded product (ap_weights / ap_rows; tiles it cannot hold fall back to ap_direct), 1 = interval moments
    // from the mu prefix sums (ap_moments_kernel: cost grows with the intervals crossed, not with a table size), 2 = the reference's quadrature
    // everywhere; default: 1 for k grids so fine that a 2 % distortion at the last k crosses more than half the knots the weight tables hold
    int ap_mode = 0;
    double *PA1 = nullptr, *PA2 = nullptr, *PA2T = nullptr, *PA3 = nullptr;  // operand rows of the first-stage GEMMs (prep_rows_kernel)
    double* coefT = nullptr;                 // FFTLog coefficients, cosmology-contiguous [2][129][B]
    double2* SAD = nullptr;                  // anti-diagonal partial sums S[AD_CH][B][nbasis + nbasis13][257]
    double *A22 = nullptr, *A13 = nullptr;   // synthesis rows of the P22 basis [B][BAS22][KSYN] and of P13 [B][10][KLIN]
    double *ACF = nullptr, *ALC = nullptr;   // ... of the weighted xi basis [B][BASC][KSYN] and of C11 / Cct [B][2 Nl][KLIN]
    double *Y22 = nullptr, *YCF = nullptr;   // synthesised basis rows [B][BAS22][Nk], [B][BASC][NS]
    // linear post-AP operators (window / binning / chained), stored K-major for gemm_rows_kernel
    struct Op { int nl_out, nx_out, nl_in, nx_in, ld; double* dev; int st_op; };  // st_op >= 0: matrix used for the Pstl rows instead
    std::vector<Op> ops;
    int pipeline_op = -1;
    int ntr = 1;                    // tracers per likelihood point: batch entry = walker * ntr + tracer (eftb_set_tracers)
    std::vector<int> tracer_ops;    // per-tracer pipeline operators (eftb_set_pipeline_operator_tracer), empty = pipeline_op for all
    // likelihood of the LOGP stage (eftb_set_likelihood)
    int like_ndata = 0, like_nG = 0, jeffreys = 0;
    int like_nl = 0, like_nx = 0;   // template-block shape the data index was validated against (checked again when the LOGP stage launches)
    // input / output guards: kernels raise flags in mapped page-locked memory (status[0]: 1 + index of a cosmology whose P_lin is
    // non-finite or non-positive at its last two samples; status[1]: 1 + index of a cosmology with a non-finite P_l, EFTB_O_CHECK_FINITE)
    // One pair per rotating set of the staged API (status[2 q], status[2 q + 1]: raised and cleared with step q's own results, whatever runs
    // beside it) and one pair (slot NSETS) for runs on the engine's own buffers (eftb_put / eftb_run / eftb_eval_batch).
    int* status = nullptr;
    int status_slot = 16;           // = NSETS: pair the kernels of the next launch raise (eftb_run_staged: the step's set)
    bool check_finite = false;
    std::vector<double> like_host;  // eftb_eval_logp_batch: D2H landing block [B][MARG_OUT]
    int* like_index = nullptr;
    double *like_data = nullptr, *like_invcov = nullptr, *like_mu = nullptr, *like_sinv = nullptr;
    double *like_V = nullptr, *like_U = nullptr;  // LOGP scratch: V and U = V C^-1, packed [walkers][nG + 1][ndata]
    // parameter draws against the current template block (eftb_draws_logp / eftb_draws_reduce).  draw_gen counts the changes of what the
    // per-walker Gram matrices depend on (the template block, the likelihood, the tracers): every run or eftb_put that writes TEMPL / TEMPLN
    // bumps it, and so do eftb_set_likelihood, eftb_set_tracers, eftb_set_template_dims and eftb_apply_operator.  The Gram block is rebuilt
    // when its generation is not the current one.
    unsigned long long draw_gen = 1, gram_gen = 0;
    int gram_C = 0;                 // walkers the cached Gram block holds
    bool templ_ok = false;          // the block holds templates: not after a direct-P_l run, nor once a staged step has rotated the blocks
    bool run_direct = false;        // the synchronous run being launched took the direct-P_l path (set by launch_stages_impl)
    size_t templ_elems = 0;         // doubles at the front of TEMPL written by the last template-producing run / eftb_put
    double *drw_A = nullptr, *drw_U = nullptr, *drw_W = nullptr, *drw_in = nullptr, *drw_inn = nullptr, *drw_out = nullptr;  // grown on demand
    size_t drw_A_cap = 0, drw_U_cap = 0, drw_W_cap = 0, drw_in_cap = 0, drw_inn_cap = 0, drw_out_cap = 0, drw_off_cap = 0;
    long long* drw_off = nullptr;
    std::vector<double> drw_host;   // eftb_draws_logp: D2H landing block [N][MARG_OUT]
    bool drw_lds = false;           // every draw kernel instantiation has opted in to the large dynamic LDS (draws_lds_optin)
    // draw recipes (eftb_set_draw_recipe): [0] of eftb_draws_logp_params, [1] of eftb_draws_reduce_params.  coef [nterms] and the int table
    // rowstart | ent | tstart | pack | slot (RecipeTab) live on the device; set = false: none (never set, withdrawn, or dropped)
    struct Recipe {
        bool set = false, nnlo = false;
        int P = 0, ng1 = 0, nterms = 0, nnz = 0, ntr_used = 0;
        double* coef = nullptr;
        int* tab = nullptr;
        // the derivative of the terms (kind 0; eftb_draws_logp_grad_params): dcoef [ndt], dtab = pstart | dent | dpack | erow (RecipeGradTab)
        int ndt = 0;
        double* dcoef = nullptr;
        int* dtab = nullptr;
        // the second derivative of the terms (kind 0; eftb_draws_logp_hess_params): hcoef [nh], htab = hstart | hent | hpack (RecipeHessTab)
        int nh = 0;
        double* hcoef = nullptr;
        int* htab = nullptr;
    } recipe[2];
    double* drw_theta = nullptr;    // theta [N][P] then f [C][ntr] of a params call
    size_t drw_theta_cap = 0;
    double* drw_grad = nullptr;     // eftb_draws_logp_grad_params: d ln P / d theta [N][P]
    size_t drw_grad_cap = 0;
    double* drw_hess = nullptr;     // eftb_draws_logp_hess_params: d2 ln P / d theta d theta [N][P][P]
    size_t drw_hess_cap = 0;
    // data sets sharing the likelihood's covariance (eftb_set_likelihood_datasets): dset_D [M][ndata] and dset_Ud = D C^-1; dset_gen counts
    // their changes.  eftb_draws_logp_params_datasets keeps Wg [G][J1][J1] of its last group table (grp_tab: walker [G] | dataset [G], on the
    // host and on the device) and reuses it while draw_gen, dset_gen and the table are those it was built from (grp_draw_gen = 0: none)
    int dset_M = 0;
    unsigned long long dset_gen = 1, grp_draw_gen = 0, grp_dset_gen = 0;
    double *dset_D = nullptr, *dset_Ud = nullptr, *drw_Wg = nullptr;
    size_t dset_D_cap = 0, dset_Ud_cap = 0, drw_Wg_cap = 0, drw_gtab_cap = 0;
    int* drw_gtab = nullptr;
    std::vector<int> grp_tab;
    std::vector<double> grp_f;      // f [G][ntr] of a groups call, expanded from f [C][ntr]
    // eftb_draws_sample_params: z and b [N][S][nG], chi2 [N][S], the coefficient rows [N S][ntr][24] / [N S][ntr][3], P_l [N S][ntr][nl][nx]
    // and the offsets times S of the reduce launch; grown on demand
    double *smp_z = nullptr, *smp_b = nullptr, *smp_chi2 = nullptr, *smp_coef = nullptr, *smp_coefn = nullptr, *smp_plk = nullptr;
    size_t smp_z_cap = 0, smp_b_cap = 0, smp_chi2_cap = 0, smp_coef_cap = 0, smp_coefn_cap = 0, smp_plk_cap = 0, smp_off_cap = 0;
    long long* smp_off = nullptr;
    std::vector<long long> smp_off_host;
    // eftb_draws_chain_params: one launch's slice of step [N][Tc][P] and lnu [N][Tc], the prior table [4][RECIPE_MAXP], the accept counts
    // [N], and the launch's stored states [N][kstride][P] and records [N][kstride][MARG_OUT] with their D2H landing blocks; grown on demand
    double *chn_step = nullptr, *chn_lnu = nullptr, *chn_pri = nullptr, *chn_chain = nullptr, *chn_rec = nullptr;
    size_t chn_step_cap = 0, chn_lnu_cap = 0, chn_pri_cap = 0, chn_chain_cap = 0, chn_rec_cap = 0, chn_nacc_cap = 0;
    long long* chn_nacc = nullptr;
    std::vector<double> chn_host_chain, chn_host_rec;
    std::vector<long long> chn_host_nacc;
    // eftb_draws_temper_params, which shares the chain call's buffers: beta [TEMPER_MAXR], one launch's slice of lnu_swap [ladders][events][R - 1],
    // the swap counts [ladders][max(R - 1, 1)] and the sums of ln P [N], with the landing block of the counts; grown on demand
    double *tmp_beta = nullptr, *tmp_lnus = nullptr, *tmp_sums = nullptr;
    size_t tmp_beta_cap = 0, tmp_lnus_cap = 0, tmp_sums_cap = 0, tmp_nswap_cap = 0;
    long long* tmp_nswap = nullptr;
    std::vector<long long> tmp_host_nswap;
    // eftb_draws_ensemble_params, which shares the chain call's buffers (z goes where step goes, lnq where lnu goes): one launch's slice of
    // pick [N][Tc]; grown on demand
    int* ens_pick = nullptr;
    size_t ens_pick_cap = 0;
    // EFTB_O_GRAPH / EFTB_GRAPH=1: whole-pipeline runs (masks that start at PREP) are captured once into a HIP graph per launch
    // state and replayed -- one host call per step instead of ~30, for hosts whose cores are busy or throttled.  Off by default: on
    // ROCm 7.2 the replay is 2-3 % slower than the plain launches when the host keeps up (0.566 vs 0.553 ms per 128, 0.169 vs 0.144 ms at B = 1)
    struct GraphEntry {
        int mask, B, cur_nl, cur_nx;
        unsigned long long epoch;
        const double *templ, *talt, *templn;
        hipGraph_t graph;
        hipGraphExec_t exec;
        const double *post_templ, *post_talt, *post_templn;  // state after the run
        int post_nl, post_nx;
    };
    std::vector<GraphEntry> graphs;
    unsigned long long epoch = 0;  // bumped by every setter that can change what launch_stages launches
    bool use_graphs = false;
    // Back-to-back asynchronous runs: the first stage of run i+1 (P11 spline + FFTLog, 20 us, inputs only) goes to its own stream and
    // overlaps the tail of run i (resum / AP) -- it waits for evInFree, recorded once run i no longer reads P11 / the coefficients
    hipStream_t pre = nullptr;
    hipEvent_t evPrep = nullptr, evInFree = nullptr;
    bool prep_overlap = true, inputs_settled = false;  // EFTB_PREP_OVERLAP=0 disables; inputs_settled: set by eftb_run only
    // back half (spline, AP, reduce) of run i on its own stream beside the resummation of run i+1 (EFTB_AP_OVERLAP=1): three template
    // blocks rotate (work block of this run, work block of the previous run = AP output of this one, AP output of the previous run)
    hipStream_t back = nullptr;
    hipEvent_t evResum = nullptr, evBack[2] = {nullptr, nullptr};
    double* T3 = nullptr;
    double *TaltN = nullptr, *T3N = nullptr;  // the same rotation for the NNLO template block (with_NNLO steps on the three-stream layout)
    bool ap_overlap = true, back_pending = false, allow_back = false;  // EFTB_AP_OVERLAP=0 disables
    unsigned back_step = 0;
    hipStream_t opstream = nullptr;  // where the operator launchers put their kernels (null: the main stream)
    // direct-P_l runs in the three-stream layout keep their FRONT (operand rows, first-stage products, anti-diagonal sums, synthesis rows, Q(f):
    // functions of the inputs alone) on the side stream, one run ahead of the rest of the look-ahead chain (syntheses, contraction, operand
    // build): two sets of everything the front writes, swapped per run
    struct FrontSet {
        double *PA1 = nullptr, *PA2 = nullptr, *PA2T = nullptr, *PA3 = nullptr, *coefT = nullptr, *A22 = nullptr, *A13 = nullptr, *ACF = nullptr, *ALC = nullptr;
        double *P11 = nullptr, *COEF = nullptr, *XY = nullptr, *Q = nullptr;
        double2* SAD = nullptr;
    } alt;
    hipEvent_t evFront = nullptr, evFrontFree[2] = {nullptr, nullptr};  // this run's front is done (side stream); the readers of front set [slot] are done
    unsigned front_step = 0;
    bool prev_front_side = false;
    bool ap_plk_fused = false;          // the AP stage of direct-P_l runs as ap_plk_fused_kernel (k grids whose tables fit the LDS; EFTB_AP_PLK_FUSED=0: ap_prefix + ap_plk_mom)
    bool ap_plk_nodes = false;          // EFTB_AP_PLK_NODES=1: the AP stage of direct-P_l runs as the node quadrature (ap_plk_kernel, round 3) instead of the moment form
    double* PLK0 = nullptr;             // direct-P_l runs with a PROJECT stage: P_l [B][Nl][Nk] as the AP stage leaves it (the operator then takes ONE row per cosmology)
    bool plk_direct = false;            // EFTB_O_PLK_DIRECT: whole-pipeline runs that end in REDUCE contract with the bias first (regroup_plk_kernel)
    int cur_nl = 0, cur_nx = 0;  // shape of the template block
    int resum_splits = 1;
    int Nn = 0;
    double* sm2 = nullptr;  // s^-2 row scale of Cct
    double* sm4 = nullptr;  // s^-4 row scale of CctNNLO
    double* XB = nullptr;  // optiresum: BAO-extracted copies of C11 [B][Nl][80], Cct [B][Nl][80], Cloopl [B][Nl][12][80], in this order
    double *coef2 = nullptr, *coefT2 = nullptr;  // dual_coef: FFTLog coefficients of the xi-space pieces (layouts of EFTB_B_COEF / coefT)
    double *ZC = nullptr, *ZC2 = nullptr;  // with_nnlo: zeros standing in for C11 [B][Nl][80] / Cloopl [B][Nl][12][80] in the NNLO pass of Resum.Ps

    // ---- staged-step state (everything above: state of an evaluation, whoever launches it) ----
    // Pipelined sampler steps (eftb_stage_inputs / eftb_run_staged / eftb_fetch_back): four sets of the per-step inputs (PIN, F, DA,
    // H, BIAS, GROWS) and outputs (PLK, LOGP) -- up to three launched and not yet fetched, one whose results are being fetched / refilled
    static constexpr int NSETS = 16; // rotating sets of per-launch inputs / outputs: the host may run fifteen steps ahead of the step it fetches (round 3: 8; a step's way from
                                     // the staging block to the fetched P_l is four pipeline stages long since the direct-P_l runs: four sets left bubbles)
    double* setbuf[NSETS][EFTB_B_COUNT] = {{nullptr}};
    double* setblock[NSETS] = {};   // one contiguous input block per set (PIN, F, DA, H, BIAS, GROWS at stage_off[])
    double* orig[EFTB_B_COUNT] = {nullptr};              // the engine's own buffers, current until the first staged run
    size_t stage_off[EFTB_B_COUNT] = {0};
    // page-locked staging, one block per STEP (a launch may carry several queued steps -- see SubCmd -- so staging blocks and device sets
    // rotate separately: slot = step % NSLOT, set = launch % NSETS)
    static constexpr int NSLOT = 32;
    double* stage_host[NSLOT] = {};
    size_t stage_elems = 0;
    hipStream_t cpy = nullptr;
    static constexpr int NLRING = 64;       // ring of the upload events, by launch number (a staging block is refilled NSLOT steps <= NSLOT launches later)
    hipEvent_t evStagedR[NLRING] = {}, evStagedAllR[NLRING] = {};
    hipEvent_t evSetDone[NSETS] = {};
    // Latency mode (a sampler whose next step depends on this step's P_l: nothing is queued behind the step being staged).  eftb_stage_inputs
    // finds the GPU idle -> this set's step runs on ONE queue (every cross-queue hand-over costs 15-18 us of dispatch latency, and there is no
    // neighbouring step to overlap with), the first kernel reads P_lin straight from the page-locked staging block (the 0.2 MB device copy
    // follows off the critical path; only the few KB of f / DA / H / bias are waited for, copied on the compute queue itself), and P_l is
    // written to mapped host memory by the kernel that forms it (no DMA phase).  (Measured and dropped: the AP tables beside the resummation
    // instead of beside the loop chain -- the chain gained 20 us, the resummation lost 39.)
    bool latency_auto = true;           // EFTB_LATENCY_MODE=0 disables
    bool set_latency[NSETS] = {};        // the launch on this set is a latency-mode step (evStagedAllR: the whole staging block has been uploaded; evStagedR: the part its first kernels wait for)
    bool lat_run = false;                // the run being launched is a latency-mode step
    double* plk_host_out = nullptr;      // where the kernel that forms P_l stores it besides the device buffer (PlkExit::stored; null: nowhere)
    bool plk_host_written = false;      // the kernel that formed the final P_l of the last launch also stored it to plk_host_out
    bool upload_on_side = true;         // EFTB_UPLOAD_ON_SIDE=0: staged uploads always on the copy stream
    int cur_set = 0;                    // set of the launch issued last (NSETS - 1 before the first)
    // staged sets keep P_l in device memory: with a communicator RCCL sends from it; without one the step's last stream copies it to page-locked
    // host memory with the DMA engine (plk_host) -- measured 0.447 ms per step against 0.455 ms with REDUCE writing mapped host memory over PCIe
    // from its waves
    double* plk_host[NSETS] = {};
    // RCCL gather (multi-GPU batches)
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    double* gathered = nullptr;
    double* gathered2[NSETS] = {};  // the gathered block rotates through three buffers: the root reads step i while steps i + 1, i + 2 are exchanged
    hipEvent_t evGath2[NSETS] = {};
    // the root's gathered block is copied on to page-locked host memory by the DMA engine, in line behind the exchange (no host call blocks on
    // the transfer): eftb_fetch_gathered / eftb_gathered_view read it there
    double* gath_host[NSETS] = {};
    hipEvent_t evGathHost[NSETS] = {};
    size_t gath_elems[NSETS] = {};
    int gath_set[NSETS];  // (all NSETS after eftb_create) set whose P_l exchange `slot` carries (its flags are checked when the gathered block is handed out; NSETS: the engine's own buffers)
    static_assert(NSETS == 16, "status_slot's default names NSETS");
    int gather_slot = 0;
    // Submission thread (EFTB_O_SUBMIT_THREAD, default on).  A staged step costs the host 50-95 us of HIP calls (nine kernel launches, ~20 event
    // records / waits) on top of ~30 us of validation and copies into the staging block -- more than the 0.12 ms the GPU needs for a direct-P_l
    // step of 128.  So while earlier steps are still in flight, eftb_stage_inputs only fills the staging block and eftb_run_staged only QUEUES the
    // step: this thread issues the upload kernel and every launch of the step (exactly the code the caller's thread runs otherwise), and the
    // caller goes on to the next step's inputs.  A step that finds the engine quiescent and the GPU idle (a dependent sampler's step) is issued by the
    // caller itself, as before: no hand-over latency.  Every other entry point waits until the queue is empty (sub_drain), so the engine's state
    // is only ever touched by one thread at a time; the queue and the per-step completion records are the only shared data.
    // Coalescing: steps that are still queued when the submission thread gets to them leave as ONE launch chain (their staging blocks are gathered
    // into one device set, row after row; each step's results are its rows of the set's output blocks).  At 128 cosmologies every kernel of a
    // step is a single ragged round of waves; two or four steps together cost far less than two or four launches (measured: 0.108 ms per 128 at 256
    // against 0.126).  Needs eftb_config.step_batch < max_batch (the device state is sized for max_batch; a step brings at most step_batch).
    struct SubCmd { int slot, mask, B, has_rows; unsigned long long step; double* out; size_t out_count; };  // out: the caller's page-locked destination of this step's P_l (eftb_set_step_output), or null
    static constexpr int SUBQ = 64;          // ring of queued steps (at most NSLOT - 1 can be pending: every step owns a staging block)
    SubCmd sub_ring[SUBQ];
    std::atomic<unsigned long long> sub_tail{0};   // commands pushed (caller's thread)
    std::atomic<unsigned long long> sub_head{0};   // commands completed (submission thread)
    std::atomic<bool> sub_flush{false};            // eftb_flush: what is queued leaves now (the flow control does not wait for a full group); cleared once the queue is empty
    std::atomic<bool> sub_sleeping{false}, sub_stop{false}, sub_hold{false};   // sub_hold (EFTB_O_SUBMIT_HOLD, tests): queued steps are not taken until it is cleared
    std::mutex sub_mx;
    std::condition_variable sub_cv;
    std::thread sub_thread;
    int sub_mode = 1;   // 0: the caller issues every step; 1: queued unless the engine is quiescent and the GPU idle; 2: always queued (tests)
    bool sub_started = false;
    static constexpr int SUBREC = 64;        // records of the last steps: where the step's rows are, rc + message of its launch (surface when the step is fetched)
    struct StepRec { int set, row, B, rc, nl, nx; unsigned long long launch; double* out; };
    StepRec rec[SUBREC] = {};
    char sub_err[SUBREC][256] = {};
    // what the rings rely on:
    // eftb_stage_inputs reads rec[] of the step that used the staging block last, NSLOT steps back, and a fetch that of a step < NSETS back
    static_assert(NSLOT <= SUBREC && NSETS <= SUBREC, "rec[] / sub_err[] must still hold the record of a staging block's last step");
    // every queued step owns a staging block, so at most NSLOT - 1 are pending in sub_ring[]
    static_assert(NSLOT - 1 < SUBQ, "sub_ring[] must hold every pending step");
    // launch_finished reads lring_set[] of the launches in flight: fewer than NSETS (sub_inflight's clamp; a set is reused behind its event)
    static_assert(NSETS <= NLRING, "lring_set[] must hold the set of every launch in flight");
    // eftb_stage_inputs waits on evStagedR / evStagedAllR [launch % NLRING] of that step's launch: every launch carries a step, so it is at
    // most NSLOT launches back and its ring slot has not been recorded again
    static_assert(NSLOT < NLRING, "the upload events of a staging block's last launch must not have been reused");
    // sub_main's group, launch_upload's and copy_out's per-step arrays, and the argument of stage_gather_kernel
    static_assert(MAX_UPLOAD_SEGS <= (int)(sizeof(StageSegs::s) / sizeof(StageSeg)), "a launch of MAX_COALESCE steps must fit the upload kernel's segment list");
    int coalesce_max = 1;                    // steps per launch at most (EFTB_COALESCE; 1 unless step_batch < max_batch)
    int sub_low = 2;                         // ... and below which it launches whatever is queued at once (EFTB_SUB_LOW); between the two it waits for a full group
    int sub_inflight = 4;                    // launches the submission thread keeps in flight before it lets the queue grow (EFTB_SUB_INFLIGHT)
    unsigned long long launch_seq = 0;       // staged launches issued so far (issuing thread)
    unsigned long long launch_done = 0;      // ... of which known to have finished (issuing thread's view)
    int lring_set[NLRING] = {};              // set of launch (seq % NLRING)
    std::atomic<unsigned long long> steps_launched{0};  // staged steps whose launch has been issued (by either thread), in order
    unsigned long long steps_submitted = 0;   // staged steps handed in so far (caller's thread) = what eftb_fetch_back counts `back` from
    int stg_slot = -1, stg_B = 0, stg_rows = 0;  // inputs staged into block stg_slot, waiting for eftb_run_staged
    double* stg_out = nullptr;                   // eftb_set_step_output: where the P_l of the step launched NEXT goes (the caller's page-locked array), ...
    size_t stg_out_count = 0;                    // ... which holds this many doubles
    bool stg_inline = false, stg_lat = false;    // ... to be issued by the caller's thread (engine quiescent, GPU idle), as a latency-mode step
    unsigned long long slot_step[NSLOT] = {}; // 1 + the step that used the staging block last (0: never used): its launch must be over before the block is refilled
    bool slot_latency[NSLOT] = {};            // ... which was a latency-mode step (its first kernel read P_lin from the block itself)
    size_t slot_off[EFTB_B_COUNT] = {0};      // layout of a staging block (one step: step_batch rows per array)
    size_t slot_elems = 0;
    unsigned long long launch_n = 0;          // (statistics: launches that carried the issue_n steps)
    // completion words of the staged sets in mapped page-locked memory: the step's last stream writes 1 + its step number behind everything else
    // (hipStreamWriteValue64), so the fetch of a step polls plain memory -- a hipEventQuery loop on the caller's thread takes the runtime's locks
    // thousands of times per step and slows the submission thread's launches down (measured: no gain from the thread at all with the event spin)
    volatile unsigned long long* set_done = nullptr;
    unsigned long long set_word[NSETS] = {};  // 1 + the launch whose completion write was enqueued for the set (else the set's event is what to wait for)
    unsigned long long set_cword[NSETS] = {}; // ... whose compute-done write was (set_done[NSETS + q])
    bool plk_dma = true;                      // EFTB_PLK_DMA=0: P_l of a pipelined launch through copy16_kernel instead of the DMA engine
    bool done_words = true;                   // EFTB_DONE_WORDS=0: event queries (A/B); also the fall-back when the write command is refused
    // EFTB_O_STEP_TRACE: GPU timestamps (timing events) at nine points of every staged direct-P_l launch -- upload start, front end, synthesis
    // start, operand build end, resummation start / end, spline start, AP end, copy-out end -- on their own streams: an undistorted timeline of
    // the pipelined loop (rocprofv3 doubles the host's launch cost, and under it the host, not the GPU, sets the pace); tools/step_trace.py
    static constexpr int NTP = 12, NTRACE = 64;   // (points 9-11: inside the front -- upload end, first-stage products end, anti-diagonal sums end)
    hipEvent_t evTrace[NTRACE][NTP] = {};
    hipEvent_t evTraceBase = nullptr;
    int trace_B[NTRACE] = {};
    unsigned long long trace_launch[NTRACE] = {};
    bool trace_on = false;
    int trace_slot = -1;      // ring slot of the launch being issued (-1: not traced)
    unsigned long long trace_n = 0;
    // EFTB_SUB_STATS=1: host time the issuing thread spends per step (printed by eftb_destroy)
    bool sub_stats = false;
    double issue_ns = 0.0, fill_ns = 0.0, wait_ns = 0.0;
    unsigned long long issue_n = 0, inline_n = 0;
    // eftb_draws_drag_params, which shares the chain call's buffers (its records are pairs): the pairs' walkers [2][G], frac [T], the sums [N][2]
    // and the final pairs of records [N][2][MARG_OUT]; grown on demand.  Behind
    // everything else: the fields that the submission thread and the callers share keep the places, and the cache lines, they had
    int* drg_pair = nullptr;
    double *drg_frac = nullptr, *drg_sums = nullptr, *drg_fin = nullptr;
    size_t drg_pair_cap = 0, drg_frac_cap = 0, drg_sums_cap = 0, drg_fin_cap = 0;
    std::vector<int> drg_host_pair;
    bool drg_lds = false;  // the LDS opt-in of its kernel is done
    std::vector<double> drg_host_fin;
    // eftb_draws_hmc_params, which shares the chain call's buffers (chn_step holds a launch's momenta): one launch's slice of eps [N][Tc], the
    // factors [N][P][P] and the launch's ratios [N][Tc] with their landing block; grown on demand
    double *hmc_eps = nullptr, *hmc_fac = nullptr, *hmc_ratio = nullptr;
    size_t hmc_eps_cap = 0, hmc_fac_cap = 0, hmc_ratio_cap = 0;
    std::vector<double> hmc_host_fac, hmc_host_ratio;
    bool hmc_lds = false;  // the LDS opt-in of its kernel is done
};

static void sub_stop_thread(eftb_engine* e);
static inline void sub_drain(eftb_engine* e);   // every entry point but the staged-step calls first lets the submission thread finish its queue

// RCCL is resolved lazily so that single-GPU users never load it
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;

static int rccl_load() {
    if (g_rccl.handle) return 0;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail("cannot load librccl.so: %s", dlerror());
#define RSYM(field, name)                                                 \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name)); \
    if (!g_rccl.field) return fail("librccl.so lacks %s", name);
    RSYM(GetUniqueId, "ncclGetUniqueId")
    RSYM(CommInitRank, "ncclCommInitRank")
    RSYM(CommDestroy, "ncclCommDestroy")
    RSYM(GroupStart, "ncclGroupStart")
    RSYM(GroupEnd, "ncclGroupEnd")
    RSYM(Send, "ncclSend")
    RSYM(Recv, "ncclRecv")
    RSYM(GetErrorString, "ncclGetErrorString")
#undef RSYM
    g_rccl.handle = h;
    return 0;
}

#define NCCLCHK(expr)                                                                            \
    do {                                                                                         \
        ncclResult_t _r = (expr);                                                                \
        if (_r != ncclSuccess) return fail("%s failed: %s", #expr, g_rccl.GetErrorString(_r));   \
    } while (0)

static inline void trace_point(eftb_engine* e, int p, hipStream_t st) {
    if (e->trace_slot >= 0) (void)hipEventRecord(e->evTrace[e->trace_slot][p], st);
}

static inline size_t kpad(int n) { return (size_t)(n + SYN_KPAD - 1) / SYN_KPAD * SYN_KPAD; }  // K of a first-stage GEMM: padded like the synthesis tables

// loop FFTLog size of the configuration (eftb_config.nfft, 0 = 256): nh = NFFT / 2, NPOW = 2 nh + 1 powers, NCH = nh + 1 independent coefficients
static inline int cfg_nh(const eftb_config& c) { return c.nfft ? c.nfft / 2 : NHALF; }
static inline int cfg_npow(const eftb_config& c) { return 2 * cfg_nh(c) + 1; }
static inline int cfg_nch(const eftb_config& c) { return cfg_nh(c) + 1; }

static size_t need_table_bytes(const eftb_config& c, int id) {
    const size_t D = sizeof(double);
    const int Nn = 2 * c.NIR * c.Na;
    switch (id) {
        case EFTB_T_K: return D * c.Nk;
        case EFTB_T_S: return D * NS;
        case EFTB_T_LNKIN: return D * c.Nkin;
        case EFTB_T_SKT: return D * kpad(c.Nkin) * c.Nk;
        case EFTB_T_GCT: case EFTB_T_ECT: return D * kpad(c.Nkin + c.ntail) * 2 * cfg_nch(c);
        case EFTB_T_LNXTAIL: return D * c.ntail;
        case EFTB_T_AD: return 2 * D * (size_t)(c.nbasis + (c.with_resum ? c.nbasis13 : 0)) * cfg_npow(c) * (cfg_nh(c) + 2);
        case EFTB_T_EXP22: return D * 28 * BAS22;
        case EFTB_T_EXPC: return c.with_resum ? D * (size_t)c.Nl * 38 * BASC : 0;
        case EFTB_T_MLJ: return c.with_resum ? 2 * D * c.Nl * cfg_npow(c) : 0;
        case EFTB_T_LINVEC: return 2 * D * (size_t)(10 + (c.with_resum ? (c.with_nnlo ? 3 : 2) * c.Nl : 0)) * cfg_nch(c);  // M13, Mcf11, Mcfct (, McfctNNLO)
        case EFTB_T_SYNK: return D * (size_t)ksyn_of(cfg_nh(c)) * c.Nk;
        case EFTB_T_LINK: return D * (size_t)klin_of(cfg_nh(c)) * c.Nk;
        case EFTB_T_SYNS: return c.with_resum ? D * (size_t)ksyn_of(cfg_nh(c)) * NS : 0;
        case EFTB_T_LINS: return c.with_resum ? D * (size_t)klin_of(cfg_nh(c)) * NS : 0;
        case EFTB_T_L11: return D * c.Nl * 3;
        case EFTB_T_LCT: return D * c.Nl * 6;
        case EFTB_T_L22: return D * c.Nl * 28;
        case EFTB_T_L13: return D * c.Nl * 10;
        case EFTB_T_GRP: return sizeof(int32_t) * 38 * 2;
        case EFTB_T_BXT: return c.with_resum ? D * kpad(c.Nkin + c.nxtail) * 2 * NS : 0;
        case EFTB_T_TYT: return 0;  // (unused id)
        case EFTB_T_LNXXTAIL: return c.with_resum ? D * c.nxtail : 0;
        case EFTB_T_WQLAST2: return c.with_resum ? D * (c.nxtail_lo ? 4 : 2) : 0;  // (+ the first two weights for the low tail)
        case EFTB_T_QPOLY: return c.with_resum ? D * 2 * c.Nl * c.Nl * Nn * 15 : 0;
        case EFTB_T_H: return c.with_resum ? D * c.Na * NS * c.Nk : 0;
        case EFTB_T_RSBASIS: case EFTB_T_RSBASISS: return c.with_resum ? D * RS_NB * 16 : 0;
        case EFTB_T_RSROWS: return c.with_resum ? sizeof(int32_t) * 2 * RS3_ROWS : 0;  // Nl = 3: X part, Y part per row; Nl = 2: the first 80
        case EFTB_T_MU: case EFTB_T_WMU: return c.with_ap ? D * c.nmu : 0;
        case EFTB_T_LEGMU: return c.with_ap ? D * c.Nl * c.nmu : 0;
        case EFTB_T_SPBAND: return c.with_ap ? D * (size_t)(2 * SPL_HB + 1) * c.Nk : 0;
        case EFTB_T_SPCBAND: return c.with_ap ? D * (size_t)(2 * SPL_HB + 1) * c.Nk : 0;
        case EFTB_T_SPLOCAL: return c.with_ap ? D * (size_t)16 * c.Nk : 0;
        case EFTB_T_APFID: return c.with_ap ? D * 2 : 0;
        case EFTB_T_LCTN: return c.with_nnlo ? D * c.Nl * 6 : 0;
        case EFTB_T_BAO: return c.optiresum && c.with_resum ? D * (2 * NS + 4) : 0;
        case EFTB_T_GCT2: case EFTB_T_GCT2T: return c.dual_coef ? D * kpad(c.Nkin + c.ntail) * 2 * cfg_nch(c) : 0;
        case EFTB_T_QEPOLY: return c.with_resum && c.Nl == 3 ? D * 2 * c.Nl * c.Nl * RSD_NN * 15 : 0;  // (direct-P_l runs: Q(f) in the closed-form basis)
    }
    return 0;
}

static size_t need_buffer_elems(const eftb_config& c, int id) {
    const size_t B = c.max_batch;
    const int Nn = 2 * c.NIR * c.Na;
    switch (id) {
        case EFTB_B_PIN: return B * c.Nkin;
        case EFTB_B_F: case EFTB_B_DA: case EFTB_B_H: return B;
        case EFTB_B_P11: return B * c.Nk;
        case EFTB_B_P22: return B * 28 * c.Nk;
        case EFTB_B_P13: return B * 10 * c.Nk;
        case EFTB_B_C11: case EFTB_B_CCT: return c.with_resum ? B * c.Nl * NS : 0;
        case EFTB_B_CC: return c.with_resum ? B * c.Nl * 38 * NS : 0;
        case EFTB_B_CLOOPL: return c.with_resum ? B * c.Nl * 12 * NS : 0;
        case EFTB_B_TEMPL: return B * c.Nl * NROW * c.Nk;
        case EFTB_B_XY: return c.with_resum ? B * 2 * NS : 0;
        case EFTB_B_Q: return c.with_resum ? B * 2 * c.Nl * c.Nl * Nn : 0;
        case EFTB_B_BIAS: return B * NROW;
        case EFTB_B_PLK: return B * c.Nl * c.Nk;
        case EFTB_B_COEF: return B * 2 * cfg_nch(c);
        case EFTB_B_GROWS: return B * MARG_NG1 * NROW;
        case EFTB_B_LOGP: return B * MARG_OUT;
        case EFTB_B_CCTN: return c.with_nnlo && c.with_resum ? B * c.Nl * NS : 0;
        case EFTB_B_TEMPLN: return c.with_nnlo ? B * c.Nl * NROW * c.Nk : 0;
        case EFTB_B_BIASN: return c.with_nnlo ? B * 3 : 0;
        case EFTB_B_GROWSN: return c.with_nnlo ? B * MARG_NG1 * 3 : 0;
    }
    return 0;
}

template <typename T>
static inline const T* tb(const eftb_engine* e, int id) { return static_cast<const T*>(e->tab[id]); }

// out[row][x] = sum_q A[row][q] Tab[q][x] on the FP64 matrix cores (synth_kernel); rows = (group, member).  The requested
// syntheses of a stage set are queued into one SynthBatch and launched together.
static void queue_synth(SynthBatch& sb, const double* A, long long a_group, int groups, int rpg, int K, const double* Tab, int X, double* out,
                        long long o_group, const double* gscale, const double* xscale) {
    SynthDesc& d = sb.p[sb.n];
    d.A = A; d.Tab = Tab; d.out = out; d.gscale = gscale; d.xscale = xscale;
    d.a_group = a_group; d.o_group = o_group; d.M = groups * rpg; d.rpg = rpg; d.K = K; d.X = X;
    d.wgx = (X + 63) / 64;
    d.wg_end = (sb.n ? sb.p[sb.n - 1].wg_end : 0) + d.wgx * ((d.M + 31) / 32);
    ++sb.n;
}

static void launch_synth(hipStream_t st, const SynthBatch& sb) {
    if (sb.n) hipLaunchKernelGGL(synth_kernel, dim3(sb.p[sb.n - 1].wg_end), dim3(256), 0, st, sb);
}

// the same batch on gemm_direct_kernel (one wave per 16 x 32 tile, no LDS): for problems with few rows -- the first-stage products
// (every K a multiple of 16: plan_stages)
static void launch_gemm_direct(hipStream_t st, SynthBatch sb) {
    int end = 0;
    for (int i = 0; i < sb.n; ++i) {
        SynthDesc& d = sb.p[i];
        d.wgx = (d.X + 31) / 32;
        end += d.wgx * ((d.M + 15) / 16);
        d.wg_end = end;
    }
    if (sb.n) hipLaunchKernelGGL((gemm_direct_kernel<4>), dim3(end), dim3(256), 0, st, sb);  // four waves split K
}

// one of a pair of entry points onto the same body: the FFTLog size compiled in at NFFT = 256 (no size argument), read at run time otherwise
template <typename... P, typename... A>
static void launch_nh(void (*fixed)(P...), void (*any)(P..., int), int nh, dim3 grid, dim3 block, hipStream_t st, A... args) {
    if (nh == NHALF) hipLaunchKernelGGL(fixed, grid, block, 0, st, args...);
    else hipLaunchKernelGGL(any, grid, block, 0, st, args..., nh);
}

// a draw kernel's pair of instantiations: TWO where a walker has more than 64 columns (J1 of them, the data row included)
template <typename... P, typename... A>
static void launch_two(void (*one)(P...), void (*two)(P...), int J1, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
    if (J1 > 64) hipLaunchKernelGGL(two, grid, block, lds, st, args...);
    else hipLaunchKernelGGL(one, grid, block, lds, st, args...);
}

// anti-diagonal sums of every loop matrix for the batch (shared by the k-space and the xi-space pieces), then the
// synthesis rows selected by `sets` (build_rows_kernel); the basis is 7 + 2 or 7 (plan_stages)
static void launch_antidiag_rows(eftb_engine* e, hipStream_t st, int B, int sets, const double* coef, const double* coefT, bool contracted = false) {
    const eftb_config& c = e->c;
    const int nc = c.nbasis + (c.with_resum ? c.nbasis13 : 0);
    const int nh = cfg_nh(c), npow = 2 * nh + 1;
    // antidiag: one workgroup of NW waves per (j', 64 cosmologies); build_rows: ceil(NPOW / 64) x 64 lanes per (cosmology, half) -- 5 at NFFT = 256
    const dim3 grid(npow, (B + 63) / 64), rgrid(B, 2, (npow + 63) / 64);
#define AD_ARGS B, c.max_batch, coefT, tb<double2>(e, EFTB_T_AD), e->SAD
#define ROW_ARGS sets, c.max_batch, c.Nl, c.with_nnlo ? 3 : 2, c.nbasis, coef, e->SAD, tb<double2>(e, EFTB_T_MLJ), tb<double2>(e, EFTB_T_LINVEC), e->A22, e->A13, \
                 e->ACF, e->ALC
#define PLK_ARGS c.max_batch, c.nbasis, coef, e->SAD, tb<double2>(e, EFTB_T_MLJ), tb<double2>(e, EFTB_T_LINVEC), e->buf[EFTB_B_BIAS], e->buf[EFTB_B_F], \
                 tb<double>(e, EFTB_T_L11), tb<double>(e, EFTB_T_LCT), tb<double>(e, EFTB_T_L22), tb<double>(e, EFTB_T_L13), tb<int>(e, EFTB_T_GRP), \
                 tb<double>(e, EFTB_T_EXP22), tb<double>(e, EFTB_T_EXPC), e->A22, e->A13, e->ACF, e->ALC
    if ((sets & 0x10) && !(contracted && WHATIF_SKIP(4))) {  // two waves per workgroup: two free wave slots on a CU are found sooner than four
        if (nc == 9) launch_nh(antidiag_kernel<9, 2>, antidiag_nh_kernel<9, 2>, nh, grid, dim3(128), st, AD_ARGS);
        else launch_nh(antidiag_kernel<7, 2>, antidiag_nh_kernel<7, 2>, nh, grid, dim3(128), st, AD_ARGS);
    }
    if (contracted) trace_point(e, 11, st);
    if (contracted && nc == 9) {  // direct-P_l runs: the rows contracted with the bias before the synthesis (3 per cosmology and space)
        if (!WHATIF_SKIP(8)) launch_nh(build_rows_plk_kernel<9>, build_rows_plk_nh_kernel<9>, nh, rgrid, dim3(64), st, PLK_ARGS);
    } else if (nc == 9) launch_nh(build_rows_kernel<9>, build_rows_nh_kernel<9>, nh, rgrid, dim3(64), st, ROW_ARGS);
    else launch_nh(build_rows_kernel<7>, build_rows_nh_kernel<7>, nh, rgrid, dim3(64), st, ROW_ARGS);
#undef AD_ARGS
#undef ROW_ARGS
#undef PLK_ARGS
}

// out[w][a][r][x] = sum_{l,k} T[w][l][r][k] * opT[(l,k)][(a,x)] on the FP64 matrix cores; the block changes shape
// Entries t0, t0 + tstride, ... of the batch go through operator `id`; with commit the block pointers are swapped and the
// block takes the operator's output shape (the last of a set of per-tracer launches commits).
static int launch_operator(eftb_engine* e, int id, int B, int t0 = 0, int tstride = 1, bool commit = true) {
    if (id < 0 || id >= (int)e->ops.size()) return fail("operator id %d out of range", id);
    const eftb_engine::Op& o = e->ops[id];
    if (o.nl_in != e->cur_nl || o.nx_in != e->cur_nx)
        return fail("operator %d expects templates [%d][24][%d], the block is [%d][24][%d]", id, o.nl_in, o.nx_in, e->cur_nl, e->cur_nx);
    // rows [r0, r0 + nr) of every (cosmology, multipole) through matrix `m`
    auto launch = [&](const eftb_engine::Op& m, int r0, int nr) {
        GemmDesc g{};
        const long long bin = (long long)o.nl_in * NROW * o.nx_in, bout = (long long)o.nl_out * NROW * o.nx_out;
        g.A = e->buf[EFTB_B_TEMPL] + (size_t)t0 * bin + (size_t)r0 * o.nx_in; g.a_group = bin * tstride; g.a_row = o.nx_in;
        g.a_seg = (long long)NROW * o.nx_in;
        g.rows = ((B - t0 + tstride - 1) / tstride) * nr; g.rows_per_group = nr; g.nseg = o.nl_in; g.kseg = o.nx_in;
        g.B = m.dev; g.ldb = m.ld; g.ncols = o.nl_out * o.nx_out;
        g.C = e->Talt + (size_t)t0 * bout + (size_t)r0 * o.nx_out; g.c_group = bout * tstride; g.c_row = o.nx_out;
        g.c_colgroup = (long long)NROW * o.nx_out;
        g.cols_per_group = o.nx_out;
        if (g.ncols <= 16 * GN_MAXT)  // few output columns: K split over the waves, 16-row workgroups
            hipLaunchKernelGGL(gemm_narrow_kernel, dim3((g.rows + 15) / 16, 1), dim3(256), 0, (e->opstream ? e->opstream : e->stream), g, GemmZ{});
        else
            hipLaunchKernelGGL(gemm_rows_kernel, dim3((g.rows + 63) / 64, (g.ncols + 255) / 256), dim3(256), GEMM_LDS, (e->opstream ? e->opstream : e->stream), g);
    };
    if (o.st_op < 0) launch(o, 0, NROW);
    else {
        launch(o, 0, NROW - 3);                 // P11l, Pctl, Ploopl
        launch(e->ops[o.st_op], NROW - 3, 3);   // Pstl (window_st / fiberst semantics of the reference)
    }
    if (!commit) return 0;
    std::swap(e->buf[EFTB_B_TEMPL], e->Talt);
    e->cur_nl = o.nl_out;
    e->cur_nx = o.nx_out;
    return 0;
}

// PROJECT stage: one operator for every entry, or one per tracer on the strided subsets
static int launch_pipeline_operator(eftb_engine* e, int B) {
    if (e->tracer_ops.empty()) {
        if (e->pipeline_op < 0) return fail("eftb_run: stage PROJECT needs eftb_set_pipeline_operator");
        return launch_operator(e, e->pipeline_op, B);
    }
    if (B % e->ntr) return fail("eftb_run: batch %d is not a multiple of the %d tracers per likelihood point", B, e->ntr);
    const eftb_engine::Op& o = e->ops[e->tracer_ops[0]];
    bool one_launch = e->ntr <= GN_MAXZ && o.nl_out * o.nx_out <= 16 * GN_MAXT;
    for (int t = 0; t < e->ntr; ++t) one_launch = one_launch && e->ops[e->tracer_ops[t]].st_op < 0;
    if (!one_launch) {
        for (int t = 0; t < e->ntr; ++t)
            if (int rc = launch_operator(e, e->tracer_ops[t], B, t, e->ntr, t == e->ntr - 1)) return rc;
        return 0;
    }
    // narrow outputs, one matrix per tracer: the tracers are the z dimension of a single launch
    if (o.nl_in != e->cur_nl || o.nx_in != e->cur_nx)
        return fail("the tracers' operators expect templates [%d][24][%d], the block is [%d][24][%d]", o.nl_in, o.nx_in, e->cur_nl, e->cur_nx);
    GemmDesc g{};
    GemmZ z{};
    const long long bin = (long long)o.nl_in * NROW * o.nx_in, bout = (long long)o.nl_out * NROW * o.nx_out;
    g.A = e->buf[EFTB_B_TEMPL]; g.a_group = bin * e->ntr; g.a_row = o.nx_in; g.a_seg = (long long)NROW * o.nx_in;
    g.rows = (B / e->ntr) * NROW; g.rows_per_group = NROW; g.nseg = o.nl_in; g.kseg = o.nx_in;
    g.B = o.dev; g.ldb = o.ld; g.ncols = o.nl_out * o.nx_out;
    g.C = e->Talt; g.c_group = bout * e->ntr; g.c_row = o.nx_out; g.c_colgroup = (long long)NROW * o.nx_out; g.cols_per_group = o.nx_out;
    for (int t = 0; t < e->ntr; ++t) z.B[t] = e->ops[e->tracer_ops[t]].dev;
    z.a_off = bin;
    z.c_off = bout;
    hipLaunchKernelGGL(gemm_narrow_kernel, dim3((g.rows + 15) / 16, 1, e->ntr), dim3(256), 0, (e->opstream ? e->opstream : e->stream), g, z);
    std::swap(e->buf[EFTB_B_TEMPL], e->Talt);
    e->cur_nl = o.nl_out;
    e->cur_nx = o.nx_out;
    return 0;
}

// PROJECT stage of a direct-P_l run: the same operators on ONE row per cosmology, P_l [B][Nl][Nk] (PLK0) -> EFTB_B_PLK [B][nl_out][nx_out]
static int launch_pipeline_operator_plk(eftb_engine* e, int B, hipStream_t st) {
    const bool per_tracer = !e->tracer_ops.empty();
    if (per_tracer && (B % e->ntr)) return fail("eftb_run: batch %d is not a multiple of the %d tracers per likelihood point", B, e->ntr);
    const int nz = per_tracer ? e->ntr : 1;
    const eftb_engine::Op& o = e->ops[per_tracer ? e->tracer_ops[0] : e->pipeline_op];
    GemmDesc g{};
    GemmZ z{};
    const long long bin = (long long)o.nl_in * o.nx_in, bout = (long long)o.nl_out * o.nx_out;
    g.A = e->PLK0; g.a_group = bin * nz; g.a_row = 0; g.a_seg = o.nx_in;
    g.rows = B / nz; g.rows_per_group = 1; g.nseg = o.nl_in; g.kseg = o.nx_in;
    g.B = o.dev; g.ldb = o.ld; g.ncols = o.nl_out * o.nx_out;
    g.C = e->buf[EFTB_B_PLK]; g.c_group = bout * nz; g.c_row = 0; g.c_colgroup = o.nx_out; g.cols_per_group = o.nx_out;
    if (g.ncols <= 16 * GN_MAXT && nz <= GN_MAXZ) {  // few output columns: K split over the waves, 16-row workgroups; the tracers are the z dimension
        for (int t = 0; t < nz; ++t) z.B[t] = e->ops[per_tracer ? e->tracer_ops[t] : e->pipeline_op].dev;
        z.a_off = bin;
        z.c_off = bout;
        hipLaunchKernelGGL(gemm_narrow_kernel, dim3((g.rows + 15) / 16, 1, nz), dim3(256), 0, st, g, z);
    } else {
        for (int t = 0; t < nz; ++t) {
            GemmDesc gt = g;
            gt.A = g.A + (size_t)t * bin;
            gt.C = g.C + (size_t)t * bout;
            gt.B = e->ops[per_tracer ? e->tracer_ops[t] : e->pipeline_op].dev;
            if (gt.ncols <= 16 * GN_MAXT) hipLaunchKernelGGL(gemm_narrow_kernel, dim3((gt.rows + 15) / 16, 1), dim3(256), 0, st, gt, GemmZ{});
            else hipLaunchKernelGGL(gemm_rows_kernel, dim3((gt.rows + 63) / 64, (gt.ncols + 255) / 256), dim3(256), GEMM_LDS, st, gt);
        }
    }
    e->cur_nl = o.nl_out;
    e->cur_nx = o.nx_out;
    return 0;
}

static void launch_prep_rows(eftb_engine* e, hipStream_t st, int B, bool first, bool ir) {
    const eftb_config& c = e->c;
#define PREP_ARGS c.Nkin, c.ntail, c.nxtail, (int)kpad(c.Nkin), (int)kpad(c.Nkin + c.ntail), (int)kpad(c.Nkin + c.nxtail), c.max_batch, e->buf[EFTB_B_PIN], \
                  tb<double>(e, EFTB_T_LNKIN), tb<double>(e, EFTB_T_LNXTAIL), tb<double>(e, EFTB_T_LNXXTAIL), tb<double>(e, EFTB_T_WQLAST2), \
                  first ? e->PA1 : nullptr, e->PA2, e->PA2T, ir ? e->PA3 : nullptr, e->status + 2 * e->status_slot
    if (c.ntail_lo || c.nxtail_lo)  // input grid above the FFTLog's xmin: low-k tails too
        hipLaunchKernelGGL(prep_rows_lo_kernel, dim3(B), dim3(256), (size_t)c.Nkin * sizeof(double), st, PREP_ARGS, c.ntail_lo, c.nxtail_lo);
    else
        hipLaunchKernelGGL(prep_rows_kernel, dim3(B), dim3(256), (size_t)c.Nkin * sizeof(double), st, PREP_ARGS);
#undef PREP_ARGS
}

// the front of a direct-P_l run on the side stream: all operand rows and Q(f) in one launch (with the low-k tails where the grid has them)
static void launch_prep_rows_qf(eftb_engine* e, hipStream_t st, int B) {
    const eftb_config& c = e->c;
#define PRQ_ARGS B, c.Nkin, c.ntail, c.nxtail, (int)kpad(c.Nkin), (int)kpad(c.Nkin + c.ntail), (int)kpad(c.Nkin + c.nxtail), c.max_batch, e->buf[EFTB_B_PIN], \
                 tb<double>(e, EFTB_T_LNKIN), tb<double>(e, EFTB_T_LNXTAIL), tb<double>(e, EFTB_T_LNXXTAIL), tb<double>(e, EFTB_T_WQLAST2), e->PA1, e->PA2, e->PA2T, e->PA3, \
                 e->status + 2 * e->status_slot, c.Nl * c.Nl * RSD_NN, e->buf[EFTB_B_F], tb<double>(e, EFTB_T_QEPOLY), e->buf[EFTB_B_Q]
    if (WHATIF_SKIP(1)) return;
    if (c.ntail_lo || c.nxtail_lo)
        hipLaunchKernelGGL(prep_rows_qf_lo_kernel, dim3(2 * B), dim3(256), (size_t)c.Nkin * sizeof(double), st, PRQ_ARGS, c.ntail_lo, c.nxtail_lo);
    else
        hipLaunchKernelGGL(prep_rows_qf_kernel, dim3(2 * B), dim3(256), (size_t)c.Nkin * sizeof(double), st, PRQ_ARGS);
#undef PRQ_ARGS
}

static void queue_xy(eftb_engine* e, SynthBatch& sb, int B) {  // X(s), Y(s) [B][2][80] = [Pin | tail'] (BX BY ; TX TY)
    const eftb_config& c = e->c;
    queue_synth(sb, e->PA3, 0, 1, B, (int)kpad(c.Nkin + c.nxtail), tb<double>(e, EFTB_T_BXT), 2 * NS, e->buf[EFTB_B_XY], 0, nullptr, nullptr);
}

// Resum.IRFilters + Resum.makeQ: X, Y (operand rows + one GEMM, unless the first stage of this run already produced them) and Q(f)
// (a direct-P_l run reads Q(f) in the closed-form basis of its resummation: Q_e(f), 48 entries per (a, l, l') where Q(f) has 96 -- each run
// evaluates the block that its own resummation reads)
static void launch_irfilter(eftb_engine* e, hipStream_t st, int B, bool xy = true, bool direct = false) {
    const eftb_config& c = e->c;
    if (xy) {
        launch_prep_rows(e, st, B, false, true);
        SynthBatch sb{};
        queue_xy(e, sb, B);
        launch_gemm_direct(st, sb);
    }
    hipLaunchKernelGGL(qf_kernel, dim3(B), dim3(256), 0, st, c.Nl * c.Nl * (direct ? RSD_NN : e->Nn), e->buf[EFTB_B_F],
                       tb<double>(e, direct ? EFTB_T_QEPOLY : EFTB_T_QPOLY), e->buf[EFTB_B_Q]);
}

static int timer_begin(eftb_engine* e, hipStream_t st, int kind);
static void timer_end(eftb_engine* e, hipStream_t st, int tslot);

// per-s A operand of the Nl = 3 resummation from Q(f), X(s), Y(s) (resum_as_kernel)
static void launch_resum_as(eftb_engine* e, hipStream_t st, int B) {
    const eftb_config& c = e->c;
    hipLaunchKernelGGL(resum_as_kernel, dim3(B, 4), dim3(256), 0, st, e->Nn, c.NIR, c.Na, e->buf[EFTB_B_Q], tb<double>(e, EFTB_T_RSBASISS),
                       tb<int>(e, EFTB_T_RSROWS), e->buf[EFTB_B_XY], e->RSAS);
}

static void launch_ap_prefix(eftb_engine* e, hipStream_t st, int B, bool weights = true) {
    const eftb_config& c = e->c;
    double** b = e->buf;
    const size_t pflds = ((size_t)(1 + 2 * c.Nl) * c.nmu + (size_t)c.Nl * c.Nl * 4 * 8) * sizeof(double);
#define PF_ARGS c.nmu, b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), tb<double>(e, EFTB_T_MU), tb<double>(e, EFTB_T_WMU), \
                tb<double>(e, EFTB_T_LEGMU), e->APP, e->APR
    if (c.Nl == 3) hipLaunchKernelGGL((ap_prefix_kernel<3>), dim3(B), dim3(320), pflds, st, PF_ARGS);
    else hipLaunchKernelGGL((ap_prefix_kernel<2>), dim3(B), dim3(128), pflds, st, PF_ARGS);
#undef PF_ARGS
    if (e->ap_mode != 0 || !weights) return;
    // knot weights of the fast path: inputs only as well, so they ride with the prefix sums (look-ahead stream in overlapped runs)
    const dim3 wgrid(((c.Nk + 63) / 64) * B);  // flat: (k tile, cosmology) decoded XCD-aware in the kernel
    const size_t wlds = ((size_t)c.Nk + c.nmu + (size_t)c.Nl * c.Nl * 4 * 64) * sizeof(double);  // knots, roots, the waves' coefficient windows
#define APW_ARGS c.Nk, c.nmu, tb<double>(e, EFTB_T_K), b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), tb<double>(e, EFTB_T_MU), e->APP, e->APR, \
                 tb<double>(e, EFTB_T_SPLOCAL), e->APW, e->API, e->APM
    const int tslot = timer_begin(e, st, 2);
    if (c.Nl == 3) hipLaunchKernelGGL((ap_weights_kernel<3>), wgrid, dim3(192), wlds, st, APW_ARGS);
    else hipLaunchKernelGGL((ap_weights_kernel<2>), wgrid, dim3(128), wlds, st, APW_ARGS);
    timer_end(e, st, tslot);
#undef APW_ARGS
}

// nnlo_pass: the linear stages (RESUM / AP / PROJECT) once more, on the NNLO block (pointers swapped in by launch_stages)
// P_l = sum_row b_row T[l][row] as two FMA chains split at this row (the row split of ap_rows_kernel's half waves), everywhere
static inline int reduce_msplit(const eftb_config& c) { return c.with_ap ? ((c.ap_stochastic ? NROW : 21) + 1) / 2 : NROW / 2; }

// after a synchronous run: a run that writes the template block is a new generation of it (eftb_draws_*); a direct-P_l run leaves none
static void note_templates(eftb_engine* e, int mask, int B) {
    if (!(mask & (EFTB_S_REGROUP | EFTB_S_RESUM | EFTB_S_AP | EFTB_S_PROJECT | EFTB_K_RESUM))) return;
    ++e->draw_gen;
    e->templ_ok = !e->run_direct;
    e->templ_elems = (size_t)B * e->cur_nl * NROW * e->cur_nx;
}

// the main stream picks up behind a back half that is still in flight on its own stream (see engine.back)
static inline void join_back(eftb_engine* e) {
    if (!e->back_pending) return;
    (void)hipStreamWaitEvent(e->stream, e->evBack[(e->back_step + 1) & 1], 0);  // the last one recorded
    e->back_pending = false;
}

// every stream of the engine drained (setters that replace resident tables / likelihood data)
static hipError_t sync_all(eftb_engine* e) {
    join_back(e);
    for (hipStream_t q : {e->stream, e->side, e->pre, e->back, e->cpy})
        if (q) {
            const hipError_t rc = hipStreamSynchronize(q);
            if (rc != hipSuccess) return rc;
        }
    return hipSuccess;
}

// flags raised by the kernels of finished runs (call after the runs in question have finished); reported once, then cleared.
// slot >= 0: only that pair (a staged step's own flags: the steps queued behind it keep theirs); slot < 0: every pair, after a synchronisation
static int check_status(eftb_engine* e, const char* who, int slot = -1) {
    if (!e->status) return 0;
    volatile int* s = e->status;
    const int lo = slot < 0 ? 0 : slot, hi = slot < 0 ? eftb_engine::NSETS : slot;
    int bad_in = 0, bad_out = 0;
    for (int q = lo; q <= hi; ++q) {
        if (!bad_in && !bad_out) {
            bad_in = s[2 * q];
            bad_out = s[2 * q + 1];
        }
        s[2 * q] = s[2 * q + 1] = 0;
    }
    if (!bad_in && !bad_out) return 0;
    if (bad_in)
        return fail("%s: P_lin of cosmology %d is non-finite, or not positive at its last (with a low-k tail: or first) two samples (the FFTLog power-law extrapolation needs "
                    "them positive, reference fftlog.py:146-151); the outputs of that run are invalid", who, bad_in - 1);
    return fail("%s: non-finite P_l(k) for cosmology %d (EFTB_O_CHECK_FINITE)", who, bad_out - 1);
}

static inline void cpu_pause() { __builtin_ia32_pause(); }

// bound of every spin below, in seconds
static double fetch_timeout_s() {
    static const double limit_s = getenv("EFTB_FETCH_TIMEOUT_S") ? atof(getenv("EFTB_FETCH_TIMEOUT_S")) : 60.0;
    return limit_s;
}

// The one bounded spin: polls done() with `pauses` pause instructions between polls and looks at the clock every period_mask + 1 polls (a
// poll of plain memory is a few ns, an event query a microsecond: each site brings its own period).  false: the bound ran out first, counted
// from t0.  What a time-out means is the caller's business.
template <typename Done>
static bool spin_until(Done done, unsigned period_mask, int pauses = 1, std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now()) {
    for (unsigned spins = 0; !done(); ++spins) {
        for (int i = 0; i < pauses; ++i) cpu_pause();
        if ((spins & period_mask) == period_mask && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > fetch_timeout_s()) return false;
    }
    return true;
}

// bounded spin on an event (the sampler thread is about to enqueue the next step: the wake-up latency of a blocking wait would be paid once per step)
static int spin_event(hipEvent_t ev, const char* who, const char* what) {
    hipError_t q = hipSuccess;
    if (!spin_until([&] { return (q = hipEventQuery(ev)) != hipErrorNotReady; }, 0xfff, 0))
        return fail("%s: %s did not finish within %.0f s (EFTB_FETCH_TIMEOUT_S)", who, what, fetch_timeout_s());
    return q == hipSuccess ? 0 : fail("%s: %s", who, hipGetErrorString(q));
}

// host inputs of one batch, before anything is copied: finite everywhere, P_lin positive where its logarithm is taken, distances positive
static int validate_inputs(const eftb_config& c, const char* who, int B, const double* Pin, const double* f, const double* DA, const double* H) {
    for (int w = 0; w < B; ++w) {
        const double* p = Pin + (size_t)w * c.Nkin;
        // exponent field all ones <=> Inf or NaN: an integer pass per row (the floating-point form, a sum of 0 x p[j], is one serial chain of adds per
        // row: 15 us per step of 128 on the sampler's thread against 7), the element-wise search only when it trips
        unsigned long long bad = 0;
        for (int j = 0; j < c.Nkin; ++j) {
            unsigned long long u;
            memcpy(&u, p + j, sizeof u);
            bad |= (unsigned long long)((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
        }
        if (bad)
            for (int j = 0; j < c.Nkin; ++j)
                if (!std::isfinite(p[j])) return fail("%s: Pin[%d][%d] is not finite", who, w, j);
        if (!(p[c.Nkin - 1] > 0.0) || !(p[c.Nkin - 2] > 0.0))
            return fail("%s: Pin[%d] must be positive at its last two samples (power-law extrapolation of the FFTLog, reference fftlog.py:146-151)", who, w);
        if ((c.ntail_lo || c.nxtail_lo) && (!(p[0] > 0.0) || !(p[1] > 0.0)))
            return fail("%s: Pin[%d] must be positive at its first two samples (low-k power-law extrapolation of the FFTLog, reference fftlog.py:140-145)", who, w);
        if (!std::isfinite(f[w])) return fail("%s: f[%d] is not finite", who, w);
        if (c.with_ap && (!std::isfinite(DA[w]) || !std::isfinite(H[w]) || !(DA[w] > 0.0) || !(H[w] > 0.0)))
            return fail("%s: DA[%d], H[%d] must be finite and positive", who, w, w);
    }
    return 0;
}

// adds the finished event pairs of the dominant-kernel timer to the running sum (wait = true: after a synchronisation, all of them)
static void collect_timer(eftb_engine* e, int slot, bool wait) {
    for (int t = 0; t < eftb_engine::NTIMER; ++t) {
        if ((slot >= 0 && t != slot) || !e->timer_busy[t]) continue;
        if (wait) (void)hipEventSynchronize(e->evT1[t]);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->evT0[t], e->evT1[t]) == hipSuccess) {
            e->timer_ms[e->timer_kind[t]] += ms;
            ++e->timer_n[e->timer_kind[t]];
            e->timer_cosmo[e->timer_kind[t]] += e->timer_B[t];
            e->timer_busy[t] = false;
        }
    }
}

// EFTB_O_TIME_DOMINANT: the launch that follows on `st` is bracketed with an event pair if it is this sample's turn (-> slot, or -1)
static int timer_begin(eftb_engine* e, hipStream_t st, int kind) {
    if (!e->time_dominant || !(e->time_kernel & (1 << kind)) || !e->evT0[0] || e->use_graphs || (e->time_seqk[kind]++ % (unsigned)e->time_dominant) != 0)
        return -1;  // (not under graph replay: the event records would be captured)
    const int tslot = (int)(e->timer_next++ % eftb_engine::NTIMER);
    collect_timer(e, tslot, false);
    if (e->timer_busy[tslot]) return -1;  // its previous pair has not finished: skip this sample
    e->timer_kind[tslot] = kind;
    e->timer_B[tslot] = e->launch_B;
    return hipEventRecord(e->evT0[tslot], st) == hipSuccess ? tslot : -1;
}
static void timer_end(eftb_engine* e, hipStream_t st, int tslot) {
    if (tslot >= 0 && hipEventRecord(e->evT1[tslot], st) == hipSuccess) e->timer_busy[tslot] = true;
}

// with_NNLO: CctNNLO rides in the resummation records of the first pass when the batch is large enough for unsplit s sums (the main kernel then
// accumulates PctNNLOl beside Pctl: no second resummation)
static inline bool nnlo_fusable(const eftb_engine* e) {
    const eftb_config& c = e->c;
    return c.with_resum && c.Nl == 3 && e->resum_splits == 1 && !c.optiresum;
}

// The layout of one launch_stages_impl call: every decision that follows from the mask, the configuration and the engine's state as the call
// finds it (plan_stages).  The stage functions read it and decide nothing of the kind themselves.  NOT in here: the pointers a run swaps (RSA /
// RSA2, APP / APP2, the FrontSet, T3) and the event slots (back_step, rs_step, front_step) -- those are read where they are used, after the swaps.
struct StagePlan {
    // nnlo_pass: the linear stages (RESUM / AP / PROJECT) once more, on the NNLO block (pointers swapped in by launch_stages)
    // nnlo_inline (launch_stages): this call carries the NNLO block through regrouping, resummation (fused accumulator), AP and REDUCE itself
    bool nnlo_pass, nnlo_inline;
    // The IR filters / Q(f) and the AP prefix sums depend on the inputs only: when they are part of a longer stage set they
    // run on a side stream beside the (latency-bound) loop path and are joined right before their consumers.
    // side_ap = side_ap0 && !direct (direct-P_l runs take the AP stage as the node quadrature on one row: no prefix sums, no knot weights)
    bool side_ir, side_ap0, side_ap;
    // with_NNLO: CctNNLO rides in the resummation records of the first pass when the batch is large enough for unsplit s sums (nnlo_fusable; not
    // in the NNLO pass itself): the main kernel accumulates PctNNLOl beside Pctl (no second pass)
    bool nnlo_fused;
    // cross-run overlap of the front half (see engine.pre): only for asynchronous runs whose inputs are already in place
    // (with_NNLO steps stay on one stream: with only the front half overlapped they measured 0.66 ms per 128 against 0.64 ms in line)
    bool pre_side;
    // ... and of the back half (spline, AP, reduce) on its own stream beside the next run's resummation (see engine.back)
    bool ap_side;
    // three-stream runs keep the regrouping and the operand build of the resummation on the look-ahead stream as well: the main stream
    // then carries nothing but the resummation kernels, back to back
    bool ahead;
    bool xy_in_prep;  // X, Y ride with the first-stage GEMMs
    // whole-pipeline runs regroup C22 / C13 into the resummation records directly (resum_prep_kernel): no regroup_cf_kernel, no Cloopl
    // buffer on the way (EFTB_B_CLOOPL then keeps what the last stand-alone REGROUP stage left there)
    bool fuse_cf;
    // P_l = sum_row b_row T[l][row]: two FMA chains split at msplit (the row split of ap_rows_kernel's half waves), everywhere
    int msplit;
    // REDUCE directly behind the AP stage: the bias contraction rides in the epilogue of ap_rows_kernel (and of the fallback tiles'
    // ap_direct_kernel), in the summation order of reduce_kernel(msplit) -- no separate pass over the 33 MB of AP output
    bool fuse_reduce;
    // direct-P_l runs (EFTB_O_PLK_DIRECT): the bias contraction first, then resummation and AP on ONE row per multipole (regroup_plk_kernel,
    // resum_prep_plk_kernel, resum_plk_kernel, spline / ap_rows on row 0); the template block is not produced
    // (only runs that also hold PREP, LOOPS and CF: the front of a direct run leaves CONTRACTED rows in Y22 / P13 / YCF / C11 / CCT, which is what
    // back_prep_plk_kernel reads -- a run split in front of REGROUP finds un-contracted rows there and takes the template path)
    // Round 4: also with a PROJECT stage behind AP (window / binning / chained are linear maps of the k and multipole axes that act on every row
    // alike: reference window.py:371-415, binning.py:131-162, chained.py:56-68 -- the operator takes ONE row per cosmology instead of 24) unless an
    // operator keeps a second matrix for the stochastic rows; and on every k grid (the AP stage of a direct run is the moment form on B-spline
    // pieces, which needs neither the knot-weight tables nor their grid limit).  LOGP runs stay templates-first: they need 1 + n_G contracted rows.
    bool proj_plk;  // every operator of the PROJECT stage can act on the contracted row
    bool direct_tail, direct, direct_proj;
    // ... and the per-s A operand of the Nl = 3 resummation (inputs only: Q(f), X, Y) is built on the side stream, off the chain
    bool as_side;
    // ... whose front runs a step ahead on the side stream (see FrontSet)
    bool front_side;
    // row counts of the configuration: the loop-matrix basis (7 + 2), the row lengths of the synthesis tables at this NFFT (528 / 288 at 256), the
    // rows of a template block that go through the AP stage
    int ncf, ksyn, klin, ap_nr;
};

// rows of one AP pass over a block.  nn: the NNLO block carries only the three counter-term rows 3-5 of every multipole: spline and AP touch
// those alone
struct ApRows {
    bool dir, red;
    int nr, rlo, rsel, msplit;
};
static ApRows ap_rows_of(const eftb_engine* e, const StagePlan& p, bool nn) {
    const bool moments = e->ap_mode == 1;  // (works on whole blocks: the NNLO block's zero rows stay zero)
    ApRows a;
    a.dir = p.direct && !nn;  // direct-P_l runs: row 0 of every (cosmology, l) block is the only one that goes through the stage
    a.red = p.fuse_reduce && !nn;
    a.nr = a.dir ? 1 : nn ? (moments ? 21 : 6) : p.ap_nr;
    // rows the spline data is needed for: [rlo, rlo + rsel) of every (cosmology, l) -- the counter-term rows of the NNLO block; on the fast
    // path only the rows the stage distorts (Pstl passes through unless APst: 21 of 24 rows)
    a.rlo = nn && !moments ? 3 : 0;
    a.rsel = a.dir ? 1 : nn && !moments ? 3 : (e->ap_mode == 0 ? a.nr : NROW);
    a.msplit = a.red ? p.msplit : (a.rlo + a.nr + 1) / 2;  // rows [rlo, msplit) / [msplit, nr) to the two half waves
    return a;
}

// Fills the plan and does nothing else: no HIP call, no write to the engine.  Every configuration error of a run is raised here, before the
// first launch: no half-issued run is left behind on the look-ahead streams.  (What stays with its stage: the shape of the template block as
// PROJECT and LOGP find it, which the stages in front of them set.)
static int plan_stages(const eftb_engine* e, int mask, int B, bool nnlo_pass, bool nnlo_inline, StagePlan* p) {
    const eftb_config& c = e->c;
    const int Nk = c.Nk, Nl = c.Nl;
    if ((mask & (EFTB_S_CF | EFTB_K_C22)) && !c.with_resum) return fail("eftb_run: stage CF needs with_resum=1");
    if ((mask & (EFTB_S_RESUM | EFTB_K_RESUM)) && !c.with_resum) return fail("eftb_run: stage RESUM needs with_resum=1");
    if ((mask & EFTB_K_IRFILTER) && !(mask & EFTB_S_RESUM) && !c.with_resum) return fail("eftb_run: EFTB_K_IRFILTER needs with_resum=1");
    if ((mask & EFTB_S_AP) && !c.with_ap) return fail("eftb_run: stage AP needs with_ap=1");
    if ((mask & EFTB_S_PROJECT) && e->tracer_ops.empty() && e->pipeline_op < 0) return fail("eftb_run: stage PROJECT needs eftb_set_pipeline_operator");
    if ((mask & EFTB_S_LOGP) && !e->like_ndata) return fail("eftb_run: stage LOGP needs eftb_set_likelihood");
    if ((mask & (EFTB_S_PROJECT | EFTB_S_LOGP)) && (B % e->ntr)) return fail("eftb_run: batch %d is not a multiple of the %d tracers per likelihood point", B, e->ntr);
    if ((mask & EFTB_S_LOGP) && (size_t)e->ntr * (e->like_nG + 1) * NROW * sizeof(double) > 64 * 1024)
        return fail("eftb_run: stage LOGP: %d tracers x %d rows do not fit the coefficient block in LDS", e->ntr, e->like_nG + 1);
    p->nnlo_pass = nnlo_pass;
    p->nnlo_inline = nnlo_inline;
    p->ncf = c.nbasis + (c.with_resum ? c.nbasis13 : 0);
    p->ksyn = ksyn_of(cfg_nh(c));
    p->klin = klin_of(cfg_nh(c));
    p->ap_nr = c.ap_stochastic ? NROW : 21;
    if ((mask & (EFTB_S_LOOPS | EFTB_S_CF | EFTB_K_P22 | EFTB_K_C22)) && p->ncf != 9 && p->ncf != 7)
        return fail("loop-matrix basis of dimension %d + %d is not instantiated (expected 7 + 2)", c.nbasis, c.with_resum ? c.nbasis13 : 0);
    p->side_ir = !nnlo_pass && (mask & EFTB_S_RESUM) && c.with_resum && (mask & (EFTB_S_PREP | EFTB_S_LOOPS | EFTB_S_CF | EFTB_S_REGROUP));
    p->side_ap0 = !nnlo_pass && (mask & EFTB_S_AP) && c.with_ap && (mask & (EFTB_S_PREP | EFTB_S_LOOPS | EFTB_S_CF | EFTB_S_REGROUP | EFTB_S_RESUM));
    p->nnlo_fused = c.with_nnlo && nnlo_fusable(e) && !nnlo_pass;
    p->pre_side = (mask & EFTB_S_PREP) && (mask & EFTB_S_REGROUP) && e->prep_overlap && e->inputs_settled && !e->use_graphs && !nnlo_pass &&
                  (!c.with_nnlo || nnlo_inline);
    p->ap_side = p->pre_side && e->ap_overlap && e->allow_back && (mask & EFTB_S_RESUM) && (mask & EFTB_S_AP);
    p->ahead = p->ap_side && e->RSA2;
    p->xy_in_prep = (mask & EFTB_S_PREP) && (mask & EFTB_S_RESUM) && c.with_resum && !nnlo_pass;
    p->fuse_cf = (mask & EFTB_S_REGROUP) && (mask & EFTB_S_RESUM) && c.with_resum && !c.optiresum && !c.with_nnlo && !nnlo_pass;
    p->msplit = reduce_msplit(c);
    p->fuse_reduce = (mask & EFTB_S_AP) && (mask & EFTB_S_REDUCE) && !(mask & (EFTB_S_PROJECT | EFTB_S_LOGP)) && c.with_ap && e->ap_mode == 0 &&
                     !c.with_nnlo && !nnlo_pass;
    p->proj_plk = true;
    if (mask & EFTB_S_PROJECT) {
        auto one = [&](int id) { return id >= 0 && id < (int)e->ops.size() && e->ops[id].st_op < 0 && e->ops[id].nl_in == Nl && e->ops[id].nx_in == Nk; };
        if (e->tracer_ops.empty()) p->proj_plk = one(e->pipeline_op);
        else
            for (int t = 0; t < e->ntr; ++t) p->proj_plk = p->proj_plk && one(e->tracer_ops[t]) && e->ops[e->tracer_ops[t]].nl_out == e->ops[e->tracer_ops[0]].nl_out &&
                                                           e->ops[e->tracer_ops[t]].nx_out == e->ops[e->tracer_ops[0]].nx_out;
    }
    p->direct_tail = (mask & EFTB_S_AP) && (mask & EFTB_S_REDUCE) && !(mask & EFTB_S_LOGP) && c.with_ap && !c.with_nnlo && !nnlo_pass && p->proj_plk && e->PLK0;
    p->direct = e->plk_direct && p->direct_tail && p->fuse_cf && Nl == 3 && !c.dual_coef && !e->use_graphs &&
                (mask & EFTB_S_PREP) && (mask & EFTB_S_LOOPS) && (mask & EFTB_S_CF) && (mask & EFTB_S_REGROUP) && e->RSAS;
    p->direct_proj = p->direct && (mask & EFTB_S_PROJECT);
    p->as_side = p->ahead && Nl == 3 && e->RSAS2 && !p->direct;
    p->front_side = p->direct && p->ahead && e->alt.A22 && (mask & EFTB_S_PREP) && (mask & (EFTB_S_LOOPS | EFTB_S_CF)) && p->xy_in_prep;
    p->side_ap = p->side_ap0 && !p->direct;
    // K of the first-stage products (gemm_direct_kernel: four waves split K in steps of 16): P11 and the coefficients, X and Y
    const bool xy = p->xy_in_prep || ((mask & (EFTB_S_RESUM | EFTB_K_IRFILTER)) && !nnlo_pass);
    for (int K : {(mask & EFTB_S_PREP) ? (int)kpad(c.Nkin) : 0, (mask & EFTB_S_PREP) ? (int)kpad(c.Nkin + c.ntail) : 0, xy ? (int)kpad(c.Nkin + c.nxtail) : 0})
        if (K % 16) return fail("eftb_run: K = %d of a first-stage product is not a multiple of 16", K);
    // the AP passes of this call on the fast path (the main block or, in the NNLO pass, the NNLO block; in line: both)
    for (int pass = 0; pass < ((mask & EFTB_S_AP) && e->ap_mode == 0 ? (nnlo_inline ? 2 : 1) : 0); ++pass) {
        const ApRows a = ap_rows_of(e, *p, pass ? true : nnlo_pass);
        const int nh = (a.nr - a.rlo + 1) / 2;
        if (!a.dir && (a.rlo + 2 * nh > NROW || a.msplit - a.rlo > nh || a.nr - a.msplit > nh || (nh != 2 && nh != 11 && nh != 12)))
            return fail("eftb_run: AP rows [%d, %d) split at %d do not fit the window layouts built into ap_rows_kernel", a.rlo, a.nr, a.msplit);
    }
    return 0;
}

// The cursor of a run through the five streams: where the chain's next kernel goes (st), where the front's kernels go (fst), and whether the
// chain has picked up what the side stream produced (joined: X, Y, Q(f); joined_ap: the AP tables)
struct StageRun {
    eftb_engine* e;
    int mask, B;
    StagePlan p;
    hipStream_t st, fst;
    bool joined, joined_ap;
    // `to` goes on behind what `from` holds so far (what: fork / join)
    int hand_over(hipEvent_t ev, hipStream_t from, hipStream_t to, const char* what) const {
        return hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess ? fail("eftb_run: stream %s failed", what) : 0;
    }
    int wait_on(hipStream_t s, hipEvent_t ev, const char* what = "wait") const {
        return hipStreamWaitEvent(s, ev, 0) != hipSuccess ? fail("eftb_run: stream %s failed", what) : 0;
    }
    int record(hipEvent_t ev, hipStream_t s, const char* what = "event record") const {
        return hipEventRecord(ev, s) != hipSuccess ? fail("eftb_run: %s failed", what) : 0;
    }
};

// the input-only kernels (IR filters / Q(f); AP prefix sums and knot weights) on the side stream, behind whatever the caller made it wait for
static int fork_side(StageRun& r) {
    eftb_engine* e = r.e;
    const StagePlan& p = r.p;
    if (p.side_ir) launch_irfilter(e, e->side, r.B, !p.xy_in_prep, p.direct);
    if (int rc = r.record(e->evJoin, e->side, "stream join")) return rc;
    if (p.side_ap) {
        if (p.pre_side) {
            // the AP tables alternate between two sets because the previous run's AP reads its own late (the set written here was last read
            // two runs ago: evBack)
            std::swap(e->APP, e->APP2);
            std::swap(e->APR, e->APR2);
            std::swap(e->APW, e->APW2);
            std::swap(e->API, e->API2);
            std::swap(e->APM, e->APM2);
            if (p.ap_side)  // its reader
                if (int rc = r.wait_on(e->side, e->evBack[e->back_step & 1])) return rc;
        }
        launch_ap_prefix(e, e->side, r.B);
    }
    return r.record(e->evJoinAP, e->side, "stream join");
}

// PREP: operand rows, then every first-stage product in one launch on the matrix cores: P11, the FFTLog coefficients (and their
// cosmology-contiguous transpose for the anti-diagonal pass), the second coefficient set of IRcutoff "loop" / "resum" (reference
// pybird.py:1151-1160), and X(s), Y(s) when a resummation follows in this run
static int stage_prep(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const StagePlan& p = r.p;
    const int B = r.B;
    double** b = e->buf;
    if (!(r.mask & EFTB_S_PREP)) return 0;
    const hipStream_t st0 = r.st;
    if (p.front_side) {
        // the front of this run goes to the side stream, into the set the run before the previous one used (its readers -- syntheses,
        // contraction, operand build -- have signalled evFrontFree); the rest of the chain (pre stream) picks up at the syntheses
        r.st = e->pre;
        eftb_engine::FrontSet& a = e->alt;
        std::swap(e->PA1, a.PA1); std::swap(e->PA2, a.PA2); std::swap(e->PA2T, a.PA2T); std::swap(e->PA3, a.PA3); std::swap(e->coefT, a.coefT);
        std::swap(e->A22, a.A22); std::swap(e->A13, a.A13); std::swap(e->ACF, a.ACF); std::swap(e->ALC, a.ALC); std::swap(e->SAD, a.SAD);
        std::swap(b[EFTB_B_P11], a.P11); std::swap(b[EFTB_B_COEF], a.COEF); std::swap(b[EFTB_B_XY], a.XY); std::swap(b[EFTB_B_Q], a.Q);
        ++e->epoch;  // (graphs captured earlier hold the other set's pointers)
        r.fst = e->side;
        if (int rc = r.wait_on(r.fst, e->evFrontFree[e->front_step & 1])) return rc;
        if (!e->prev_front_side)
            if (int rc = r.wait_on(r.fst, e->evInFree)) return rc;
        r.joined = r.joined_ap = true;  // (X, Y, Q(f) reach the rest of the chain with evFront; no AP tables in a direct run)
    } else if (p.pre_side) {
        r.st = e->pre;
        if (int rc = r.wait_on(r.st, e->evInFree)) return rc;
        // (X, Y of the previous run are also read by its operand build on the side stream, which evInFree does not cover)
        if (p.as_side)
            if (int rc = r.wait_on(r.st, e->evAS)) return rc;
        // the input-only kernels get their own low-priority stream beside the front half: X, Y, Q are free since the previous run built its
        // resummation operands (evInFree)
        if (p.side_ir || p.side_ap) {
            if (int rc = r.wait_on(e->side, e->evInFree)) return rc;
            if (int rc = fork_side(r)) return rc;
        }
    }
    if (!p.front_side) r.fst = r.st;
    if (p.front_side) launch_prep_rows_qf(e, r.fst, B);  // operand rows and Q(f) in one launch
    else launch_prep_rows(e, r.fst, B, true, p.xy_in_prep);
    {
        SynthBatch sb{};
        const int KP1 = (int)kpad(c.Nkin), KP2 = (int)kpad(c.Nkin + c.ntail), NC2 = 2 * cfg_nch(c);
        queue_synth(sb, e->PA1, 0, 1, B, KP1, tb<double>(e, EFTB_T_SKT), c.Nk, b[EFTB_B_P11], 0, nullptr, nullptr);
        queue_synth(sb, e->PA2, 0, 1, B, KP2, tb<double>(e, EFTB_T_GCT), NC2, b[EFTB_B_COEF], 0, nullptr, nullptr);
        queue_synth(sb, tb<double>(e, EFTB_T_ECT), KP2, NC2, 1, KP2, e->PA2T, c.max_batch, e->coefT, c.max_batch, nullptr, nullptr);
        if (c.dual_coef) {
            queue_synth(sb, e->PA2, 0, 1, B, KP2, tb<double>(e, EFTB_T_GCT2), NC2, e->coef2, 0, nullptr, nullptr);
            queue_synth(sb, tb<double>(e, EFTB_T_GCT2T), KP2, NC2, 1, KP2, e->PA2T, c.max_batch, e->coefT2, c.max_batch, nullptr, nullptr);
        }
        if (p.xy_in_prep) queue_xy(e, sb, B);
        if (!(p.front_side && WHATIF_SKIP(2))) launch_gemm_direct(r.fst, sb);
        if (p.front_side) trace_point(e, 10, r.fst);
    }
    if (p.as_side) {  // behind the AP tables on the side stream; the set written here was last read by the resummation two runs ago
        if (p.xy_in_prep)
            if (int rc = r.hand_over(e->evXY, r.st, e->side, "join")) return rc;
        std::swap(e->RSAS, e->RSAS2);
        if (int rc = r.wait_on(e->side, e->evRsDone[e->rs_step & 1])) return rc;
        launch_resum_as(e, e->side, B);
        if (int rc = r.record(e->evAS, e->side)) return rc;
    }
    // with pre_side the whole front half (first stage, anti-diagonal sums, rows, syntheses, expansions: inputs -> P22, P13, C11, Cct, CC)
    // stays on the `pre` stream; the main stream picks up at the regrouping
    if (!p.pre_side) r.st = st0;
    return 0;
}

// LOOPS / CF: the anti-diagonal sums serve both the k-space and the xi-space pieces: one pass, then the synthesis rows of
// whatever is requested (bit 0/1: quadratic rows of k / xi space, bit 2/3: single-sum rows, bit 4: the sums themselves); every synthesis of the
// requested pieces in one launch, then both expansions in one launch
static int stage_loops(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const StagePlan& p = r.p;
    const int mask = r.mask, B = r.B, Nk = c.Nk, Nl = c.Nl;
    double** b = e->buf;
    if (mask & (EFTB_S_LOOPS | EFTB_S_CF | EFTB_K_P22 | EFTB_K_C22)) {
        int sets = 0x10;
        if (mask & (EFTB_S_LOOPS | EFTB_K_P22)) sets |= 0x1;
        if (mask & EFTB_S_LOOPS) sets |= 0x4;
        if (mask & (EFTB_S_CF | EFTB_K_C22)) sets |= 0x2;
        if (mask & EFTB_S_CF) sets |= 0x8;
        if (!c.dual_coef) {
            launch_antidiag_rows(e, p.front_side ? r.fst : r.st, B, sets, b[EFTB_B_COEF], e->coefT, p.direct);
            if (p.front_side) {
                trace_point(e, 1, r.fst);
                if (int rc = r.hand_over(e->evFront, r.fst, r.st, "join")) return rc;
                trace_point(e, 2, r.st);
            }
        } else {  // k-space rows from the first coefficient set, xi-space rows from the second (the sums are recomputed in between)
            if (sets & 0x5) launch_antidiag_rows(e, r.st, B, (sets & 0x5) | 0x10, b[EFTB_B_COEF], e->coefT);
            if (sets & 0xa) launch_antidiag_rows(e, r.st, B, (sets & 0xa) | 0x10, e->coef2, e->coefT2);
        }
    }
    const hipStream_t st = r.st;
    SynthBatch sb{};
    const bool k22 = mask & (EFTB_S_LOOPS | EFTB_K_P22), c22 = mask & (EFTB_S_CF | EFTB_K_C22);
    // (only the rows in use: 7 of the 8 padded basis rows per cosmology, Nl (7 + 2) = 27 of the 32 weighted ones -- 10 % of the launch's
    // matrix-core work was padding; the padded rows of Y22 / YCF stay at their initial zeros and meet zero columns in expand_kernel)
    const int ksyn = p.ksyn, klin = p.klin;
    // (direct-P_l runs: 3 contracted rows per cosmology in each of these three -- same strides, fewer rows)
    if (k22) queue_synth(sb, e->A22, (long long)BAS22 * ksyn, B, p.direct ? 3 : c.nbasis, ksyn, tb<double>(e, EFTB_T_SYNK), Nk, e->Y22, (long long)BAS22 * Nk, nullptr, nullptr);
    if (c22) queue_synth(sb, e->ACF, (long long)BASC * ksyn, B, p.direct ? 3 : Nl * p.ncf, ksyn, tb<double>(e, EFTB_T_SYNS), NS, e->YCF, (long long)BASC * NS, nullptr, nullptr);
    if (mask & EFTB_S_LOOPS)
        queue_synth(sb, e->A13, 10LL * klin, B, p.direct ? 3 : 10, klin, tb<double>(e, EFTB_T_LINK), Nk, b[EFTB_B_P13], 10LL * Nk, b[EFTB_B_P11], nullptr);
    if (mask & EFTB_S_CF) {
        const long long ag = (c.with_nnlo ? 3LL : 2LL) * Nl * klin;
        queue_synth(sb, e->ALC, ag, B, Nl, klin, tb<double>(e, EFTB_T_LINS), NS, b[EFTB_B_C11], (long long)Nl * NS, nullptr, nullptr);
        queue_synth(sb, e->ALC + (size_t)Nl * klin, ag, B, Nl, klin, tb<double>(e, EFTB_T_LINS), NS, b[EFTB_B_CCT], (long long)Nl * NS,
                    nullptr, e->sm2);
        if (c.with_nnlo)  // makeCctNNLO (reference pybird.py:1098-1101)
            queue_synth(sb, e->ALC + (size_t)2 * Nl * klin, ag, B, Nl, klin, tb<double>(e, EFTB_T_LINS), NS, b[EFTB_B_CCTN], (long long)Nl * NS,
                        nullptr, e->sm4);
    }
    const int tslot = (mask & EFTB_S_REGROUP) ? timer_begin(e, st, 1) : -1;
    if (!(p.direct && WHATIF_SKIP(16))) launch_synth(st, sb);
    timer_end(e, st, tslot);
    if ((k22 || c22) && !p.direct) {  // (direct-P_l runs contract the basis rows themselves: regroup_plk_kernel, resum_prep_plk_kernel)
        const int n22 = k22 ? ((Nk + 63) / 64) * ((28 + EXP_RPB - 1) / EXP_RPB) * B : 0;
        const int ncf = c22 ? ((NS + 63) / 64) * ((Nl * 38 + EXP_RPB - 1) / EXP_RPB) * B : 0;
        hipLaunchKernelGGL(expand_kernel, dim3(n22 + ncf), dim3(64), 0, st, n22, Nk, B, e->Y22, tb<double>(e, EFTB_T_EXP22), b[EFTB_B_P22], Nl * 38,
                           e->YCF, c22 ? tb<double>(e, EFTB_T_EXPC) : nullptr, b[EFTB_B_CC]);
    }
    return 0;
}

// REGROUP: the template block from P11, P22, P13 (and Cloopl from CC unless the resummation regroups it itself)
static int stage_regroup(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const StagePlan& p = r.p;
    const int B = r.B, Nk = c.Nk, Nl = c.Nl;
    double** b = e->buf;
    if (p.pre_side && !p.ahead) {
        if (int rc = r.hand_over(e->evPrep, r.st, e->stream, "join")) return rc;
        r.st = e->stream;
    }
    if (p.ap_side) {
        // regroup into the block the run before the previous one left its AP output in (its readers are done: evBack)
        if (int rc = r.wait_on(r.st, e->evBack[e->back_step & 1])) return rc;
        std::swap(b[EFTB_B_TEMPL], e->T3);
        if (p.nnlo_inline) std::swap(b[EFTB_B_TEMPLN], e->T3N);
    }
    if (!(r.mask & EFTB_S_REGROUP)) return 0;
    const hipStream_t st = r.st;
    if (!p.direct)  // (regroup_plk rides in the launch of the operand build of the resummation: back_prep_plk_kernel)
        hipLaunchKernelGGL(regroup_kernel, dim3((Nk + 255) / 256, B, Nl), dim3(256), 0, st, Nk, Nl, tb<double>(e, EFTB_T_K), b[EFTB_B_F],
                           b[EFTB_B_P11], b[EFTB_B_P22], b[EFTB_B_P13], tb<double>(e, EFTB_T_L11), tb<double>(e, EFTB_T_LCT),
                           tb<double>(e, EFTB_T_L22), tb<double>(e, EFTB_T_L13), tb<int>(e, EFTB_T_GRP), b[EFTB_B_TEMPL]);
    if (c.with_nnlo)
        hipLaunchKernelGGL(nnlo_rows_kernel, dim3((Nk + 255) / 256, B, Nl), dim3(256), 0, st, Nk, Nl, tb<double>(e, EFTB_T_K), b[EFTB_B_P11],
                           tb<double>(e, EFTB_T_LCTN), b[EFTB_B_TEMPLN]);
    if (c.with_resum && !p.fuse_cf)
        hipLaunchKernelGGL(regroup_cf_kernel, dim3(12, Nl, B), dim3(128), 0, st, Nl, b[EFTB_B_F], b[EFTB_B_CC], tb<double>(e, EFTB_T_L22),
                           tb<double>(e, EFTB_T_L13), tb<int>(e, EFTB_T_GRP), b[EFTB_B_CLOOPL]);
    // nothing later in this run reads the front half's outputs (P11, coefficients, P22, P13, CC; C11 / Cct only if a resummation
    // follows): the next run's front half may overwrite them from here on
    if (!(r.mask & EFTB_S_RESUM) && !e->use_graphs && !p.nnlo_pass)
        if (int rc = r.record(e->evInFree, st)) return rc;
    return 0;
}

// RESUM (EFTB_K_IRFILTER / EFTB_K_RESUM: its two halves alone): operands from Q(f), X, Y and the CF pieces, then the main kernel
static int stage_resum(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const StagePlan& p = r.p;
    const int mask = r.mask, B = r.B, Nk = c.Nk, Nl = c.Nl;
    double** b = e->buf;
    if ((mask & EFTB_K_IRFILTER) && !(mask & EFTB_S_RESUM)) launch_irfilter(e, r.st, B);
    if (!(mask & (EFTB_S_RESUM | EFTB_K_RESUM))) return 0;
    hipStream_t st = r.st;
    const bool full = mask & EFTB_S_RESUM;  // EFTB_K_RESUM alone: only the main kernel, on the operands of an earlier full run
    const bool direct = p.direct, nnlo_pass = p.nnlo_pass;
    if (full && !p.side_ir && !nnlo_pass) launch_irfilter(e, st, B, true, direct);  // X, Y, Q(f) of the first pass stay valid
    if (!r.joined) {
        if (int rc = r.wait_on(st, e->evJoin, "join")) return rc;
        r.joined = true;
    }
    const double *c11 = b[EFTB_B_C11], *cct = b[EFTB_B_CCT], *cloopl = b[EFTB_B_CLOOPL];
    if (c.optiresum && full) {  // Resum.extractBAO (reference pybird.py:1382-1400) into scratch: the stage inputs stay as the CF stage left them
        double *x11 = e->XB, *xct = x11 + (size_t)c.max_batch * Nl * NS, *xl = xct + (size_t)c.max_batch * Nl * NS;
        hipLaunchKernelGGL(extract_bao_kernel, dim3(B * Nl), dim3(128), 0, st, tb<double>(e, EFTB_T_BAO), c11, x11);
        hipLaunchKernelGGL(extract_bao_kernel, dim3(B * Nl), dim3(128), 0, st, tb<double>(e, EFTB_T_BAO), cct, xct);
        hipLaunchKernelGGL(extract_bao_kernel, dim3(B * Nl * 12), dim3(128), 0, st, tb<double>(e, EFTB_T_BAO), cloopl, xl);
        c11 = x11; cct = xct; cloopl = xl;
    }
    // matrix-core form: polynomials as [80 | 32 x 8] x [8 x 16 points] MFMAs, one wave = 16 k x one slice of the s sum
#define RP_ARGS e->Nn, c.NIR, c.Na, b[EFTB_B_Q], tb<double>(e, EFTB_T_RSBASISS), tb<int>(e, EFTB_T_RSROWS), b[EFTB_B_XY], c11, cct, cloopl, e->RSA, e->RSC, \
        p.nnlo_fused ? b[EFTB_B_CCTN] : nullptr, p.fuse_cf ? b[EFTB_B_CC] : nullptr, b[EFTB_B_F], tb<double>(e, EFTB_T_L22), tb<double>(e, EFTB_T_L13), \
        tb<int>(e, EFTB_T_GRP)
    const dim3 rpgrid(B, p.fuse_cf ? 5 : 1);  // the fused regrouping is 38 conditional terms per record entry: spread over five workgroups
    const int rslot = e->rs_step & 1;
    if (p.ahead) {  // the operand set written here was last read by the resummation two runs ago
        std::swap(e->RSA, e->RSA2);
        std::swap(e->RSC, e->RSC2);
        if (direct) std::swap(e->RSAS, e->RSAS2);  // (here the coefficient table of resum_plk_kernel)
        if (int rc = r.wait_on(st, e->evRsDone[rslot])) return rc;
    }
    if (full && direct) {
        constexpr int nparts = 5;  // slices of the s range per cosmology (2 ... 10 measured the same since the coefficient part keeps Q(f) in registers: 20-22 us alone at 512 per launch, 8 at 128)
        const int nsl = (NS + nparts - 1) / nparts;
        const size_t plds = ((size_t)2 * 3 * nsl + 2 * nsl) * sizeof(double);
        const int nkx = (Nk + 255) / 256, nreg = nkx * B;   // (regroup: one workgroup per (256 k, cosmology), all three l)
        if (!WHATIF_SKIP(32))
            hipLaunchKernelGGL(back_prep_plk_kernel, dim3(nreg + nparts * B), dim3(BPP_THREADS), plds, st, nreg, nkx, B, nparts, Nk, Nl, tb<double>(e, EFTB_T_K), b[EFTB_B_P11], e->Y22,
                               b[EFTB_B_P13], tb<double>(e, EFTB_T_L11), tb<double>(e, EFTB_T_LCT), b[EFTB_B_BIAS], b[EFTB_B_TEMPL], c.ap_stochastic ? 1 : 0,
                               b[EFTB_B_Q], b[EFTB_B_XY], c11, cct, e->YCF, e->RSAS);
        trace_point(e, 3, st);
        if (p.front_side) {  // the last reader of this run's front set
            if (int rc = r.record(e->evFrontFree[e->front_step & 1], st)) return rc;
            ++e->front_step;
        }
    } else if (full) {
        if (Nl == 3 && !p.as_side) launch_resum_as(e, st, B);  // (in line: X, Y, Q(f) are in place behind evJoin)
        if (Nl == 3) hipLaunchKernelGGL((resum_prep_kernel<3>), rpgrid, dim3(256), 0, st, RP_ARGS);
        else hipLaunchKernelGGL((resum_prep_kernel<2>), rpgrid, dim3(256), 0, st, RP_ARGS);
    }
#undef RP_ARGS
    // C11 / Cct / Cloopl now live in the per-s records: the next run's front half may overwrite its outputs (see the regrouping)
    if (full && (mask & EFTB_S_REGROUP) && !e->use_graphs && !nnlo_pass)
        if (int rc = r.record(e->evInFree, st)) return rc;
    if (p.ahead) {
        if (int rc = r.hand_over(e->evPrep, st, e->stream, "join")) return rc;
        if (p.as_side && full)
            if (int rc = r.wait_on(e->stream, e->evAS, "join")) return rc;
        st = r.st = e->stream;
    }
    if (direct) trace_point(e, 4, st);
    const int tslot = full ? timer_begin(e, st, 0) : -1;
    const int kblocks = (Nk - c.Nklow + 63) / 64;
    int nsplit = 1;
    while (!direct && nsplit < e->resum_splits && (size_t)kblocks * 4 * B * nsplit < 2048) nsplit *= 2;
    const int schunk = (NS + nsplit - 1) / nsplit;
#define RM_ARGS Nk, c.Nklow, schunk, tb<double>(e, EFTB_T_K), tb<double>(e, EFTB_T_H), tb<double>(e, EFTB_T_RSBASIS), Nl == 3 ? e->RSAS : e->RSA, e->RSC, tb<double>(e, EFTB_T_L11), \
        tb<double>(e, nnlo_pass ? EFTB_T_LCTN : EFTB_T_LCT), b[EFTB_B_TEMPL], e->part, nsplit
    const int nkb = (Nk - (c.Nklow & ~15) + 63) / 64;  // Nl = 3: k tiles aligned to 16, (k block, cosmology) decoded from a flat index
    if (direct) {
        // two k per lane, eight slices of the s range: a wave owns all nine (l, v) of its points, a workgroup one (128 k, cosmology).  Alone at
        // B = 128 (rocprofv3, same machine and session, sets of eight coefficients): <2,8> 31.1 us, <2,10> 44.3, <2,5> 43.2, <2,4> 51.8, <1,8> 52.1;
        // <2,8> with sets of sixteen, the form that runs: 29.3; the Horner kernel it replaces, <4,4> of 3 SH waves per (256 k, l): 35.4
        const int nkd = (Nk + 64 * RSD_KPL - 1) / (64 * RSD_KPL);
        if (kblocks > 0 && !WHATIF_SKIP(64))
            hipLaunchKernelGGL((resum_plk_kernel<RSD_KPL, RSD_SH>), dim3(nkd * B), dim3(64 * RSD_SH), 0, st, Nk, c.Nklow, tb<double>(e, EFTB_T_K), tb<double>(e, EFTB_T_H),
                               e->RSAS, b[EFTB_B_TEMPL], nkd);
    } else if (kblocks > 0 && Nl == 3 && p.nnlo_fused)
        hipLaunchKernelGGL((resum_mfma_kernel<true>), dim3(nkb * B, 1, nsplit), dim3(256), 0, st, RM_ARGS, tb<double>(e, EFTB_T_LCTN), b[EFTB_B_TEMPLN], nkb);
    else if (kblocks > 0 && Nl == 3)
        hipLaunchKernelGGL((resum_mfma_kernel<false>), dim3(nkb * B, 1, nsplit), dim3(256), 0, st, RM_ARGS, nullptr, nullptr, nkb);
    else if (kblocks > 0) hipLaunchKernelGGL(resum_mfma2_kernel, dim3(kblocks, B, nsplit), dim3(256), 0, st, RM_ARGS);
#undef RM_ARGS
    if (nsplit > 1)
        hipLaunchKernelGGL(resum_sum_kernel, dim3((Nk + 255) / 256, 21 * Nl, B), dim3(256), 0, st, Nk, Nl, nsplit, e->part, b[EFTB_B_TEMPL]);
    timer_end(e, st, tslot);
    if (direct) trace_point(e, 5, st);
    if (p.ahead) {
        if (int rc = r.record(e->evRsDone[rslot], st)) return rc;
        ++e->rs_step;
    }
    return 0;
}

// the AP stage of a direct-P_l run: the contracted row `in` -> P_l, in one of three forms
static void ap_pass_plk(StageRun& r, const double* in) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const int B = r.B, Nk = c.Nk;
    const hipStream_t st = r.st;
    double** b = e->buf;
    // (a PROJECT stage follows: the stage leaves P_l in PLK0 and the operator writes the final block)
    double* const plk_dst = r.p.direct_proj ? e->PLK0 : b[EFTB_B_PLK];
    double* const plk_hst = r.p.direct_proj ? nullptr : e->plk_host_out;
    // (the tables between the nodes and the spline data: the quadrature weights and Legendre values, or the mu prefix sums and roots)
#define APK_ARGS(...) Nk, c.nmu, tb<double>(e, EFTB_T_K), b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), tb<double>(e, EFTB_T_MU), __VA_ARGS__, e->SD, \
                      tb<double>(e, EFTB_T_SPLOCAL), in, b[EFTB_B_BIAS], plk_dst, plk_hst, e->check_finite ? e->status + 2 * e->status_slot + 1 : nullptr, \
                      c.ap_stochastic ? NROW : 21
    const bool nodes = e->ap_plk_nodes, fused = !nodes && e->ap_plk_fused;
    // moment form on the contracted row (ap_plk_mom_kernel): the mu prefix sums of this cosmology batch (a function of DA, H alone) in
    // line in front of it -- the stage is ~20 us of latency-bound launches either way, and in line it needs no second set of sums
    if (!nodes && !fused) launch_ap_prefix(e, st, B, false);
    const int tslot = timer_begin(e, st, 2);
    if (nodes) {  // the node quadrature on the contracted row (ap_plk_kernel); nothing else of the stage runs
        const size_t lds = ((size_t)((Nk + 1) & ~1) + (size_t)c.nmu * 8 + 3 * APD_WMAX * 4 + 3 * 3 * 64) * sizeof(double);
        hipLaunchKernelGGL((ap_plk_kernel<3>), dim3(((Nk + 63) / 64) * B), dim3(256), lds, st, APK_ARGS(tb<double>(e, EFTB_T_WMU), tb<double>(e, EFTB_T_LEGMU)));
    } else if (fused) {
        // moment form with everything in LDS (ap_plk_fused_kernel): prefix sums, pieces and the walk in one launch
        const size_t lds = ((size_t)((Nk + 1) & ~1) + (size_t)c.nmu * (2 + 2 * 3) + 36 * 16 + (size_t)(c.nmu + 1) * 36 + (size_t)(Nk - 1) * 3 * 4) * sizeof(double);
        // one workgroup of eight waves per cosmology (22.3 us alone at B = 128, 40 at 384; two workgroups of four waves measured 22.7 / 61 -- the
        // LDS tables allow one workgroup per CU either way)
        if (!WHATIF_SKIP(256))
            hipLaunchKernelGGL((ap_plk_fused_kernel<3, 8>), dim3(B), dim3(512), lds, st, APK_ARGS(tb<double>(e, EFTB_T_WMU), tb<double>(e, EFTB_T_LEGMU)));
        trace_point(e, 7, st);
    } else {
        const size_t lds = ((size_t)Nk + c.nmu + 3 * 3 * 64) * sizeof(double);
        hipLaunchKernelGGL((ap_plk_mom_kernel<3>), dim3(((Nk + 63) / 64) * B), dim3(256), lds, st, APK_ARGS(e->APP, e->APR));
    }
#undef APK_ARGS
    timer_end(e, st, tslot);
}

// one AP pass over a template block: *pin -> *palt, then the two trade places (nn: see ApRows)
static int ap_pass(StageRun& r, bool nn, double** pin, double** palt) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    const StagePlan& p = r.p;
    const int B = r.B, Nk = c.Nk, Nl = c.Nl;
    const hipStream_t st = r.st;
    double** b = e->buf;
    const ApRows a = ap_rows_of(e, p, nn);
    const int nr = a.nr, rlo = a.rlo, msplit = a.msplit;
    const int nseries = B * Nl * a.rsel;
    if (a.dir) trace_point(e, 6, st);
    {
        const int kt = (Nk + 63) / 64;
        int ysplit = std::max(1, std::min((nseries + 15) / 16, 1024 / kt));  // ~4 workgroups per CU, each sweeping its share of the series
        if (ysplit >= 8) ysplit &= ~7;  // shares in multiples of 8: the k tiles of a share then sit on one XCD (xcd_decode)
        // (the fast path keeps the splines as B-spline coefficients -- one number per knot; the moment / quadrature forms as knot slopes)
        if (!(a.dir && WHATIF_SKIP(128)))
            hipLaunchKernelGGL(spline_kernel, dim3(kt * ysplit), dim3(256), 0, st, Nk, nseries, rlo, a.rsel, *pin, tb<double>(e, e->ap_mode == 0 || a.dir ? EFTB_T_SPCBAND : EFTB_T_SPBAND), e->SD);
    }
    if (a.dir) {
        ap_pass_plk(r, *pin);
        std::swap(*pin, *palt);
        return 0;
    }
    // prefix sums over mu per cosmology (side stream when possible), then interval moments by differences x cubic coefficients
    if (!p.side_ap && !nn) launch_ap_prefix(e, st, B);
    if (!r.joined_ap) {
        if (int rc = r.wait_on(st, e->evJoinAP, "join")) return rc;
        r.joined_ap = true;
    }
    if (e->ap_mode == 1) {
        const dim3 apgrid((Nk + 63) / 64, B, 3);
        const size_t aplds = ((size_t)Nk + c.nmu + (size_t)4 * Nl * ((nr + 2) / 3) * 64) * sizeof(double);
#define APM_ARGS Nk, c.nmu, tb<double>(e, EFTB_T_K), b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), tb<double>(e, EFTB_T_MU), e->APP, e->APR, *pin, e->SD, *palt
        if (Nl == 3 && nr == 21) hipLaunchKernelGGL((ap_moments_kernel<3, 21, 3>), apgrid, dim3(256), aplds, st, APM_ARGS);
        else if (Nl == 3) hipLaunchKernelGGL((ap_moments_kernel<3, NROW, 3>), apgrid, dim3(256), aplds, st, APM_ARGS);
        else if (nr == 21) hipLaunchKernelGGL((ap_moments_kernel<2, 21, 3>), apgrid, dim3(256), aplds, st, APM_ARGS);
        else hipLaunchKernelGGL((ap_moments_kernel<2, NROW, 3>), apgrid, dim3(256), aplds, st, APM_ARGS);
#undef APM_ARGS
        std::swap(*pin, *palt);
        return 0;
    }
    // REDUCE directly behind the AP stage (fuse_reduce): the epilogue's bias, destinations and flag
    const double* rb = a.red ? b[EFTB_B_BIAS] : nullptr;
    double* rp = a.red ? b[EFTB_B_PLK] : nullptr;
    double* rph = a.red ? e->plk_host_out : nullptr;
    int* rflag = a.red && e->check_finite ? e->status + 2 * e->status_slot + 1 : nullptr;
    if (e->ap_mode == 0) {
        // banded product of the knot weights with the spline data; rows outside [rlo, nr) are copied through
        // (nh = 2, 11 or 12 rows per half wave: the window layouts built into ap_rows_kernel, checked by plan_stages)
        const int kt2 = 2 * ((Nk + 63) / 64), nh = (nr - rlo + 1) / 2;
        const size_t lds = 0;  // (the window is a static array: 37 KB at most)
#define APR_ARGS Nk, rlo, nr, msplit, b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), e->APW, e->API, e->APM, *pin, e->SD, *palt, rb, rp, rph, rflag
#define APR_LAUNCH(NLV, NHV) hipLaunchKernelGGL((ap_rows_kernel<NLV, NHV, 2>), dim3(kt2 * B), dim3(64 * NLV), lds, st, APR_ARGS)  // (ring of two knots' weights in flight)
        if (Nl == 3 && nh == 11) APR_LAUNCH(3, 11);
        else if (Nl == 3 && nh == 12) APR_LAUNCH(3, 12);
        else if (Nl == 3) APR_LAUNCH(3, 2);
        else if (nh == 11) APR_LAUNCH(2, 11);
        else if (nh == 12) APR_LAUNCH(2, 12);
        else APR_LAUNCH(2, 2);
#undef APR_LAUNCH
#undef APR_ARGS
    }
    // the reference's own quadrature: every tile (EFTB_AP_MODE=2), or only the tiles the fast path flagged (strong distortions)
    const bool gated = e->ap_mode == 0;
    const int4* gate = gated ? e->APM : nullptr;
    const dim3 dgrid(((Nk + 63) / 64) * B);
#define APD_ARGS Nk, c.nmu, rlo, nr, tb<double>(e, EFTB_T_K), b[EFTB_B_DA], b[EFTB_B_H], tb<double>(e, EFTB_T_APFID), tb<double>(e, EFTB_T_MU), tb<double>(e, EFTB_T_WMU), \
                 tb<double>(e, EFTB_T_LEGMU), e->APR, *pin, e->SD, *palt, gate, rb, rp, rph, msplit, rflag, tb<double>(e, EFTB_T_SPLOCAL)
    if (gated && Nl == 3) hipLaunchKernelGGL((ap_direct_kernel<3, true>), dgrid, dim3(64), 0, st, APD_ARGS);
    else if (gated) hipLaunchKernelGGL((ap_direct_kernel<2, true>), dgrid, dim3(64), 0, st, APD_ARGS);
    else if (Nl == 3) hipLaunchKernelGGL((ap_direct_kernel<3, false>), dgrid, dim3(64), 0, st, APD_ARGS);
    else hipLaunchKernelGGL((ap_direct_kernel<2, false>), dgrid, dim3(64), 0, st, APD_ARGS);
#undef APD_ARGS
    std::swap(*pin, *palt);
    return 0;
}

// AP: the back half moves to its own stream in three-stream runs; one pass over the block (and one over the NNLO block it carries in line)
static int stage_ap(StageRun& r) {
    eftb_engine* e = r.e;
    const StagePlan& p = r.p;
    if (p.ap_side) {
        // (with the operands built ahead the resummation's own event -- recorded right behind it on this stream -- is the fork point: one
        // event record less on the host's path)
        const bool rs_event = p.ahead && (r.mask & EFTB_S_RESUM);
        if (int rc = rs_event ? r.wait_on(e->back, e->evRsDone[(e->rs_step + 1) & 1], "fork") : r.hand_over(e->evResum, r.st, e->back, "fork")) return rc;
        r.st = e->back;
    }
    if (!(r.mask & EFTB_S_AP)) return 0;
    if (int rc = ap_pass(r, p.nnlo_pass, &e->buf[EFTB_B_TEMPL], &e->Talt)) return rc;
    if (p.nnlo_inline)
        if (int rc = ap_pass(r, true, &e->buf[EFTB_B_TEMPLN], &e->TaltN)) return rc;
    return 0;
}

// PROJECT: the pipeline operator(s) on the template block, or on the one row per cosmology a direct-P_l run carries
static int stage_project(StageRun& r) {
    eftb_engine* e = r.e;
    if (r.mask & EFTB_S_REGROUP) {  // the block as the stages so far leave it
        e->cur_nl = e->c.Nl;
        e->cur_nx = e->c.Nk;
    }
    if (r.p.direct_proj) {
        if (int rc = launch_pipeline_operator_plk(e, r.B, r.st)) return rc;
        e->plk_host_written = false;  // (the operator writes device memory only: whoever wants P_l in host memory copies it behind the launch)
    } else if (r.mask & EFTB_S_PROJECT) {
        e->opstream = r.st;
        const int rc = launch_pipeline_operator(e, r.B);
        e->opstream = nullptr;
        if (rc) return rc;
    }
    return 0;
}

// out [rows][ndata] = A [rows][ndata] C^-1 with the likelihood's inverse covariance, on the matrix cores (LOGP stage: V, draw calls: the gathered
// templates, data sets: D -- one and the same product, so that a row of -D there is the exact negation of its row here)
static void launch_times_invcov(eftb_engine* e, hipStream_t st, const double* A, int rows, double* out) {
    const int nd = e->like_ndata;
    GemmDesc gd{};
    gd.A = A; gd.a_group = 0; gd.a_row = nd; gd.a_seg = 0; gd.rows = rows; gd.rows_per_group = rows; gd.nseg = 1; gd.kseg = nd;
    gd.B = e->like_invcov; gd.ldb = nd; gd.ncols = nd;
    gd.C = out; gd.c_group = 0; gd.c_row = nd; gd.c_colgroup = 0; gd.cols_per_group = nd;
    hipLaunchKernelGGL(gemm_narrow_kernel, dim3((gd.rows + 15) / 16, (gd.ncols + 16 * GN_MAXT - 1) / (16 * GN_MAXT)), dim3(256), 0, st, gd, GemmZ{});
}

// LOGP: V (residual and derivatives on the data vector) per walker, U = V C^-1 for all walkers in one matrix-core GEMM, then the
// (nG + 1)^2 products and the small dense solve per walker
static int stage_logp(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    double** b = e->buf;
    if (!(r.mask & EFTB_S_LOGP)) return 0;
    if (e->cur_nl != e->like_nl || e->cur_nx != e->like_nx)
        return fail("eftb_run: stage LOGP: the likelihood's data index addresses templates [%d][24][%d], the block is [%d][24][%d]", e->like_nl,
                    e->like_nx, e->cur_nl, e->cur_nx);
    const int nw = r.B / e->ntr, ng1 = e->like_nG + 1, nd = e->like_ndata;
    const size_t lds = (size_t)e->ntr * ng1 * NROW * sizeof(double);  // (the coefficient block: at most 64 KB, plan_stages)
    hipLaunchKernelGGL(marg_build_kernel, dim3(nw), dim3(256), lds, r.st, e->cur_nl, e->cur_nx, e->ntr, nd, e->like_nG, e->like_index, e->like_data,
                       b[EFTB_B_GROWS], b[EFTB_B_TEMPL], c.with_nnlo ? b[EFTB_B_GROWSN] : nullptr, c.with_nnlo ? b[EFTB_B_TEMPLN] : nullptr,
                       e->like_V);
    launch_times_invcov(e, r.st, e->like_V, nw * ng1, e->like_U);
    hipLaunchKernelGGL(marg_solve_kernel, dim3(nw), dim3(256), 0, r.st, nd, e->like_nG, e->jeffreys, e->like_mu, e->like_sinv, e->like_V, e->like_U,
                       b[EFTB_B_LOGP]);
    return 0;
}

// REDUCE: P_l = sum_row b_row T[l][row], unless the AP stage did it in its epilogue (fuse_reduce) or the run contracted first (direct)
static int stage_reduce(StageRun& r) {
    eftb_engine* e = r.e;
    const eftb_config& c = e->c;
    double** b = e->buf;
    if (!(r.mask & EFTB_S_REDUCE)) return 0;
    if (!r.p.fuse_reduce && !r.p.direct)
        hipLaunchKernelGGL(reduce_kernel, dim3((e->cur_nx + 255) / 256, e->cur_nl, r.B), dim3(256), 0, r.st, e->cur_nx, e->cur_nl, r.p.msplit, b[EFTB_B_BIAS],
                           b[EFTB_B_TEMPL], b[EFTB_B_PLK], c.with_nnlo ? nullptr : e->plk_host_out, e->check_finite && !c.with_nnlo ? e->status + 2 * e->status_slot + 1 : nullptr);
    if (c.with_nnlo)
        hipLaunchKernelGGL(reduce_nnlo_kernel, dim3((e->cur_nx + 255) / 256, e->cur_nl, r.B), dim3(256), 0, r.st, e->cur_nx, e->cur_nl, b[EFTB_B_BIASN],
                           b[EFTB_B_TEMPLN], b[EFTB_B_PLK], e->check_finite ? e->status + 2 * e->status_slot + 1 : nullptr);
    return 0;
}

// what the next run waits for: the inputs are free (unless the regrouping or the resummation said so already), the back half is done
static int stage_tail(StageRun& r) {
    eftb_engine* e = r.e;
    if (!(r.mask & EFTB_S_REGROUP) && !e->use_graphs && !r.p.nnlo_pass)
        if (int rc = r.record(e->evInFree, r.st)) return rc;
    if (r.p.ap_side) {
        if (int rc = r.record(e->evBack[e->back_step & 1], r.st)) return rc;
        ++e->back_step;
        e->back_pending = true;
    }
    if (r.mask & EFTB_S_PREP) e->prev_front_side = r.p.front_side;
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(le));
    return 0;
}

// One run of the stages in `mask` over B cosmologies: the plan, then the stages in their order.  Each stage function launches on the cursor's
// stream and moves the cursor where its part of the layout says (StageRun); launch_stages, run_stages and issue_group call this.
static int launch_stages_impl(eftb_engine* e, int mask, int B, bool nnlo_pass, bool nnlo_inline = false) {
    e->launch_B = B;
    StageRun r{e, mask, B, StagePlan{}, e->stream, e->stream, false, false};
    if (int rc = plan_stages(e, mask, B, nnlo_pass, nnlo_inline, &r.p)) return rc;
    const StagePlan& p = r.p;
    if (!p.ap_side) join_back(e);
    if (p.direct) e->run_direct = true;
    e->plk_host_written = true;
    r.joined = !p.side_ir;
    r.joined_ap = !p.side_ap;
    if ((p.side_ir || p.side_ap) && !p.pre_side) {  // (overlapped runs fork inside stage_prep, behind the waits of the look-ahead)
        if (int rc = r.hand_over(e->evFork, r.st, e->side, "fork")) return rc;
        if (int rc = fork_side(r)) return rc;
    }
    for (int (*stage)(StageRun&) : {stage_prep, stage_loops, stage_regroup, stage_resum, stage_ap, stage_project, stage_logp, stage_reduce, stage_tail})
        if (int rc = stage(r)) return rc;
    return 0;
}

static int launch_stages(eftb_engine* e, int mask, int B) {
    const eftb_config& c = e->c;
    const int lin = mask & (EFTB_S_RESUM | EFTB_S_AP | EFTB_S_PROJECT);
    if (!c.with_nnlo || !lin) return launch_stages_impl(e, mask, B, false);
    // with_NNLO: the counter-terms k^4 P11 lctNNLO go through the same linear stages as a second template block whose Pctl
    // slots carry them (reference pybird.py:1447-1458 Resum with Q[1], CctNNLO, lctNNLO; :1615 AP; window.py:399, 410):
    // everything but the tail, then the linear stages again with the NNLO operands swapped in, then LOGP / REDUCE.
    // whole-pipeline steps without PROJECT / LOGP take the three-stream layout: the NNLO block has its own three rotating blocks and
    // follows the main block through every stage inside one call
    const int whole = EFTB_S_PREP | EFTB_S_REGROUP | EFTB_S_RESUM | EFTB_S_AP;
    if (nnlo_fusable(e) && c.with_ap && (mask & whole) == whole && !(mask & (EFTB_S_PROJECT | EFTB_S_LOGP)) && e->prep_overlap && e->ap_overlap && e->inputs_settled &&
        e->allow_back && !e->use_graphs && e->T3N && e->nnlo_inline)
        return launch_stages_impl(e, mask, B, false, true);
    const int tail = mask & (EFTB_S_LOGP | EFTB_S_REDUCE);
    const int in_nl = (mask & EFTB_S_REGROUP) ? c.Nl : e->cur_nl, in_nx = (mask & EFTB_S_REGROUP) ? c.Nk : e->cur_nx;
    if (int rc = launch_stages_impl(e, mask & ~tail, B, false)) return rc;
    const int out_nl = e->cur_nl, out_nx = e->cur_nx;
    double** b = e->buf;
    auto swap_in = [&]() {
        std::swap(b[EFTB_B_TEMPL], b[EFTB_B_TEMPLN]);
        if (c.with_resum) {
            std::swap(b[EFTB_B_CCT], b[EFTB_B_CCTN]);
            std::swap(b[EFTB_B_C11], e->ZC);
            std::swap(b[EFTB_B_CLOOPL], e->ZC2);
        }
    };
    swap_in();
    e->cur_nl = in_nl;
    e->cur_nx = in_nx;
    // large batches at Nl = 3 accumulate PctNNLOl inside the resummation kernel of the first pass: only AP / PROJECT are left for the block
    const int lin2 = nnlo_fusable(e) ? (lin & ~EFTB_S_RESUM) : lin;
    const int rc = lin2 ? launch_stages_impl(e, lin2, B, true) : 0;
    swap_in();  // the same swaps undo themselves
    e->cur_nl = out_nl;
    e->cur_nx = out_nx;
    if (rc) return rc;
    return tail ? launch_stages_impl(e, tail, B, false) : 0;
}

// the likelihood's device arrays go (eftb_set_likelihood replaces them), and with them the likelihood: until the next one is complete every
// call that needs one refuses, as after eftb_set_tracers
static void drop_likelihood(eftb_engine* e) {
    for (void* p : {(void*)e->like_index, (void*)e->like_data, (void*)e->like_invcov, (void*)e->like_mu, (void*)e->like_sinv, (void*)e->like_V, (void*)e->like_U}) e->own.release(p);
    e->like_index = nullptr; e->like_data = e->like_invcov = e->like_mu = e->like_sinv = e->like_V = e->like_U = nullptr;
    e->like_ndata = e->like_nG = 0;
}

static void drop_graphs(eftb_engine* e) {
    for (auto& g : e->graphs) {
        (void)hipGraphExecDestroy(g.exec);
        (void)hipGraphDestroy(g.graph);
    }
    e->graphs.clear();
}

// launch_stages, replayed from a captured graph when the same launch state comes back (the usual case: a sampler calling the
// same pipeline step after step)
static int run_stages(eftb_engine* e, int mask, int B) {
    if (!e->use_graphs || !(mask & EFTB_S_PREP)) return launch_stages(e, mask, B);
    double** b = e->buf;
    for (auto& g : e->graphs)
        if (g.mask == mask && g.B == B && g.epoch == e->epoch && g.templ == b[EFTB_B_TEMPL] && g.talt == e->Talt && g.templn == b[EFTB_B_TEMPLN] &&
            g.cur_nl == e->cur_nl && g.cur_nx == e->cur_nx) {
            if (hipGraphLaunch(g.exec, e->stream) != hipSuccess) return fail("eftb_run: hipGraphLaunch failed");
            (void)hipEventRecord(e->evInFree, e->stream);
            b[EFTB_B_TEMPL] = const_cast<double*>(g.post_templ);
            e->Talt = const_cast<double*>(g.post_talt);
            b[EFTB_B_TEMPLN] = const_cast<double*>(g.post_templn);
            e->cur_nl = g.post_nl;
            e->cur_nx = g.post_nx;
            return 0;
        }
    eftb_engine::GraphEntry g{};
    g.mask = mask; g.B = B; g.epoch = e->epoch; g.cur_nl = e->cur_nl; g.cur_nx = e->cur_nx;
    g.templ = b[EFTB_B_TEMPL]; g.talt = e->Talt; g.templn = b[EFTB_B_TEMPLN];
    if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        e->use_graphs = false;  // this runtime cannot capture: plain launches from now on
        return launch_stages(e, mask, B);
    }
    const int rc = launch_stages(e, mask, B);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
    if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (ce != hipSuccess || !graph) {
        (void)hipGetLastError();
        e->use_graphs = false;
        return fail("eftb_run: stream capture failed (%s); graphs disabled, call again", hipGetErrorString(ce));
    }
    if (hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        e->use_graphs = false;
        return fail("eftb_run: hipGraphInstantiate failed; graphs disabled, call again");
    }
    g.graph = graph;
    g.post_templ = b[EFTB_B_TEMPL]; g.post_talt = e->Talt; g.post_templn = b[EFTB_B_TEMPLN]; g.post_nl = e->cur_nl; g.post_nx = e->cur_nx;
    if (e->graphs.size() >= 8) {
        (void)hipGraphExecDestroy(e->graphs.front().exec);
        (void)hipGraphDestroy(e->graphs.front().graph);
        e->graphs.erase(e->graphs.begin());
    }
    e->graphs.push_back(g);
    if (hipGraphLaunch(g.exec, e->stream) != hipSuccess) return fail("eftb_run: hipGraphLaunch failed");
    (void)hipEventRecord(e->evInFree, e->stream);
    return 0;
}

// Measurement: EFTB_STREAM_PAD="a,b,c,d,e" creates (and keeps) that many extra streams of the same priority in front of the main / side / look-ahead /
// back / copy stream, each touched once so that its hardware queue exists.  Which hardware queue a stream lands on decides which other streams'
// barrier packets its kernels wait behind (round 4: the copy-out of P_l on a stream of its own ran at 0.16 or 0.103 ms per step depending on how
// many streams were created before it) -- a sweep of the placement of the engine's own five streams, tools/pad_sweep.sh.
static int pad_streams(eftb_engine* e, int which, int prio) {
    const char* f = getenv("EFTB_STREAM_PAD");
    if (!f) return 0;
    int v[5] = {0, 0, 0, 0, 0};
    sscanf(f, "%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4]);
    for (int i = 0; i < v[which]; ++i) {
        hipStream_t dummy = nullptr;
        HIPCHK(own_stream(e->own, &dummy, prio));
        hipLaunchKernelGGL(wake_kernel, dim3(1), dim3(64), 0, dummy);
    }
    return 0;
}

extern "C" {

const char* eftb_last_error(void) { return g_err.c_str(); }
#ifndef EFTB_SRC_HASH
#define EFTB_SRC_HASH "unknown"
#endif
const char* eftb_source_hash(void) { return EFTB_SRC_HASH; }
const char* eftb_version(void) { return "eftbird 0.3 (gfx950, fp64: anti-diagonal loops, mfma synthesis / resummation, overlapped steps)"; }

int eftb_create(const eftb_config* cfg, eftb_engine** out) {
    if (!cfg || !out) return fail("eftb_create: null argument");
    const eftb_config& c = *cfg;
    if (c.Nl != 2 && c.Nl != 3) return fail("eftb_create: Nl must be 2 or 3 (got %d)", c.Nl);
    if (c.Nk < 8 || c.Nkin < 4 || c.max_batch < 1) return fail("eftb_create: bad dimensions Nk=%d Nkin=%d max_batch=%d", c.Nk, c.Nkin, c.max_batch);
    if (c.step_batch < 0 || c.step_batch > c.max_batch) return fail("eftb_create: step_batch=%d outside [0, max_batch=%d]", c.step_batch, c.max_batch);
    if (c.nbasis < 1 || c.nbasis > 16) return fail("eftb_create: nbasis=%d outside [1, 16]", c.nbasis);
    if (c.nfft != 0 && (c.nfft % 2 || c.nfft < 2 * NHALF || c.nfft > 512))
        return fail("eftb_create: nfft=%d unsupported (even values from 256 to 512; 0 = 256)", c.nfft);
    if (c.ntail < 0 || c.nxtail < 0 || c.ntail_lo < 0 || c.ntail_lo > c.ntail || c.nxtail_lo < 0 || c.nxtail_lo > c.nxtail ||
        ((c.ntail_lo || c.nxtail_lo) && c.Nkin < 2))
        return fail("eftb_create: tails (ntail %d, ntail_lo %d, nxtail %d, nxtail_lo %d) inconsistent", c.ntail, c.ntail_lo, c.nxtail, c.nxtail_lo);
    if (c.nxtail_lo && !c.with_resum) return fail("eftb_create: nxtail_lo needs with_resum=1");
    if (c.nbasis > BAS22 || (c.with_resum && c.Nl * (c.nbasis + c.nbasis13) > BASC)) return fail("eftb_create: loop basis %d + %d too large", c.nbasis, c.nbasis13);
    if (c.with_resum && !((c.Nl == 3 && c.NIR == 16 && c.Na == 3) || (c.Nl == 2 && c.NIR == 8 && c.Na == 2)))
        return fail("eftb_create: (Nl, NIR, Na) = (%d, %d, %d) unsupported", c.Nl, c.NIR, c.Na);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("eftb_create: no HIP device visible -- libeftbird has no CPU fallback");
    if (c.device < 0 || c.device >= ndev) return fail("eftb_create: device %d out of range (%d visible)", c.device, ndev);
    HIPCHK(hipSetDevice(c.device));
    struct Destroy { void operator()(eftb_engine* p) const { eftb_destroy(p); } };
    std::unique_ptr<eftb_engine, Destroy> guard(new eftb_engine());  // every failing exit below destroys what the engine holds so far
    eftb_engine* e = guard.get();
    e->c = c;
    for (int& g : e->gath_set) g = eftb_engine::NSETS;
    e->Nn = 2 * c.NIR * c.Na;
    e->cur_nl = c.Nl;
    e->cur_nx = c.Nk;
    if (const char* f = getenv("EFTB_GRAPH")) e->use_graphs = atoi(f) != 0;
    if (const char* f = getenv("EFTB_PREP_OVERLAP")) e->prep_overlap = atoi(f) != 0;
    if (const char* f = getenv("EFTB_NNLO_INLINE")) e->nnlo_inline = atoi(f) != 0;
    // Stream priorities.  With the regrouping and the operand build on the look-ahead stream, the look-ahead chain (a dozen latency-bound
    // kernels in series) is the critical path of a pipelined step and the resummation kernel the throughput work beside it: the chain gets
    // the high priority, the main stream the low one (measured at batch 128, evaluations/s: 266-269 k; all normal 265 k; main high and
    // look-ahead low, the round-1 assignment, 240 k; raising the wave priority of the small kernels with s_setprio lost 10 %).
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    auto prio_of = [&](const char* name, int dflt) {  // EFTB_*_PRIO = 1 low, 0 normal, -1 high
        const char* f = getenv(name);
        return !f ? dflt : (atoi(f) > 0 ? prio_lo : (atoi(f) < 0 ? prio_hi : 0));
    };
    if (int rc = pad_streams(e, 0, prio_of("EFTB_MAIN_PRIO", prio_lo))) return rc;
    HIPCHK(own_stream(e->own, &e->stream, prio_of("EFTB_MAIN_PRIO", prio_lo)));
    if (int rc = pad_streams(e, 1, prio_of("EFTB_SIDE_PRIO", 0))) return rc;
    HIPCHK(own_stream(e->own, &e->side, prio_of("EFTB_SIDE_PRIO", 0)));
    if (int rc = pad_streams(e, 2, prio_of("EFTB_PRE_PRIO", prio_hi))) return rc;
    HIPCHK(own_stream(e->own, &e->pre, prio_of("EFTB_PRE_PRIO", prio_hi)));
    HIPCHK(own_event(e->own, &e->evPrep, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evFront, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evFrontFree[0], hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evFrontFree[1], hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evXY, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evAS, hipEventDisableTiming));
    if (const char* f = getenv("EFTB_AP_OVERLAP")) e->ap_overlap = atoi(f) != 0;
    {
        int bp = prio_lo;  // measured: 290 k evaluations/s with the back half at low priority, 286 k at high, 278 k without the stream
        if (const char* f = getenv("EFTB_BACK_PRIO")) bp = atoi(f) > 0 ? prio_lo : (atoi(f) < 0 ? prio_hi : 0);
        if (int rc = pad_streams(e, 3, bp)) return rc;
        HIPCHK(own_stream(e->own, &e->back, bp));
    }
    HIPCHK(own_event(e->own, &e->evResum, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evBack[0], hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evBack[1], hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evInFree, hipEventDisableTiming));
    HIPCHK(hipEventRecord(e->evInFree, e->pre));
    HIPCHK(own_event(e->own, &e->evFork, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evJoin, hipEventDisableTiming));
    HIPCHK(own_event(e->own, &e->evJoinAP, hipEventDisableTiming));
    for (hipEvent_t& ev : e->evRsDone) HIPCHK(own_event(e->own, &ev, hipEventDisableTiming));
    for (hipEvent_t& ev : e->evRun) HIPCHK(own_event(e->own, &ev, hipEventDisableTiming));
    for (int t = 0; t < eftb_engine::NTIMER; ++t) {
        HIPCHK(own_event(e->own, &e->evT0[t]));
        HIPCHK(own_event(e->own, &e->evT1[t]));
    }
    HIPCHK(own_event(e->own, &e->ev0));
    HIPCHK(own_event(e->own, &e->ev1));
    for (int id = 0; id < EFTB_B_COUNT; ++id) {
        const size_t n = need_buffer_elems(c, id);
        e->buf_elems[id] = n;
        if (n) HIPCHK(own_dev(e->own, &e->buf[id], (n + 2) * sizeof(double), true));  // (+2: ap_rows_kernel's 16-byte window loads may end one element past a row)
    }
    const size_t B = c.max_batch;
    HIPCHK(own_dev(e->own, &e->sm2, NS * sizeof(double)));
    HIPCHK(own_dev(e->own, &e->sm4, NS * sizeof(double)));
    // scratch of the anti-diagonal pipeline; padded rows / coefficients of the synthesis rows stay zero
    {
        const size_t nc = c.nbasis + (c.with_resum ? c.nbasis13 : 0);
        // sizes of this NFFT: NCH coefficients, NPOW anti-diagonals, synthesis rows of 1 + 4 nh / 1 + 2 nh (padded)
        const size_t nch = cfg_nch(c), npow = cfg_npow(c), ksyn = ksyn_of(cfg_nh(c)), klin = klin_of(cfg_nh(c));
        struct Zeroed { double** p; size_t n; };  // (p null: not in this configuration)
        auto zeroed = [&](std::initializer_list<Zeroed> list) {
            for (const Zeroed& z : list)
                if (z.p && own_dev(e->own, z.p, z.n * sizeof(double), true) != hipSuccess) return false;
            return true;
        };
        const size_t nalc = B * (c.with_nnlo ? 3 : 2) * c.Nl * klin, nsad = 2 * (size_t)AD_CH * B * nc * npow;
        const bool rs = c.with_resum, dual = c.dual_coef;
        if (!zeroed({{&e->coefT, 2 * nch * B}, {&e->PA1, B * kpad(c.Nkin)}, {&e->PA2, B * kpad(c.Nkin + c.ntail)}, {&e->PA2T, B * kpad(c.Nkin + c.ntail)},
                     {rs ? &e->PA3 : nullptr, B * kpad(c.Nkin + c.nxtail)}, {dual ? &e->coef2 : nullptr, 2 * nch * B}, {dual ? &e->coefT2 : nullptr, 2 * nch * B},
                     {reinterpret_cast<double**>(&e->SAD), nsad}, {&e->A22, B * BAS22 * ksyn}, {&e->A13, B * 10 * klin}, {&e->Y22, B * BAS22 * c.Nk},
                     {rs ? &e->ACF : nullptr, B * BASC * ksyn}, {rs ? &e->ALC : nullptr, nalc}, {rs ? &e->YCF : nullptr, B * BASC * NS}}))
            return fail("eftb_create: out of device memory for the loop scratch");
        if (c.with_resum && c.Nl == 3 && !c.dual_coef) {  // second set of the front's outputs (direct-P_l runs, see FrontSet)
            eftb_engine::FrontSet& a = e->alt;
            if (!zeroed({{&a.coefT, 2 * nch * B}, {&a.PA1, B * kpad(c.Nkin)}, {&a.PA2, B * kpad(c.Nkin + c.ntail)}, {&a.PA2T, B * kpad(c.Nkin + c.ntail)},
                         {&a.PA3, B * kpad(c.Nkin + c.nxtail)}, {reinterpret_cast<double**>(&a.SAD), nsad}, {&a.A22, B * BAS22 * ksyn}, {&a.A13, B * 10 * klin},
                         {&a.ACF, B * BASC * ksyn}, {&a.ALC, nalc}, {&a.P11, e->buf_elems[EFTB_B_P11]}, {&a.COEF, e->buf_elems[EFTB_B_COEF]},
                         {&a.XY, e->buf_elems[EFTB_B_XY]}, {&a.Q, e->buf_elems[EFTB_B_Q]}}))
                return fail("eftb_create: out of device memory for the second front set");
        }
    }
    HIPCHK(own_dev(e->own, &e->Talt, (e->buf_elems[EFTB_B_TEMPL] + 2) * sizeof(double)));
    if (c.with_ap) {
        HIPCHK(own_dev(e->own, &e->SD, (e->buf_elems[EFTB_B_TEMPL] + 2) * sizeof(double), true));  // knot slopes of the splines, laid out like the template block
        HIPCHK(own_dev(e->own, &e->APP, (size_t)c.max_batch * (c.nmu + 1) * c.Nl * c.Nl * 4 * sizeof(double)));
        HIPCHK(own_dev(e->own, &e->APR, (size_t)c.max_batch * c.nmu * sizeof(double)));
        HIPCHK(own_dev(e->own, &e->APP2, (size_t)c.max_batch * (c.nmu + 1) * c.Nl * c.Nl * 4 * sizeof(double)));
        HIPCHK(own_dev(e->own, &e->APR2, (size_t)c.max_batch * c.nmu * sizeof(double)));
        const size_t kt = (c.Nk + 63) / 64;
        for (int q = 0; q < 2; ++q) {
            HIPCHK(own_dev(e->own, q ? &e->APW2 : &e->APW, (size_t)c.max_batch * kt * APW_DCAP * c.Nl * c.Nl * 64 * sizeof(double)));
            HIPCHK(own_dev(e->own, q ? &e->API2 : &e->API, (size_t)c.max_batch * kt * 64 * sizeof(int)));
            HIPCHK(own_dev(e->own, q ? &e->APM2 : &e->APM, (size_t)c.max_batch * 2 * kt * sizeof(int4)));  // one window record per tile of 32 k
        }
    }
    if (const char* f = getenv("EFTB_AP_PLK_NODES")) e->ap_plk_nodes = atoi(f) != 0;
    if (const char* f = getenv("EFTB_UPLOAD_ON_SIDE")) e->upload_on_side = atoi(f) != 0;
    if (const char* f = getenv("EFTB_SUBMIT_THREAD")) e->sub_mode = std::max(0, std::min(2, atoi(f)));
    HIPCHK(own_host(e->own, &e->status, 2 * (eftb_engine::NSETS + 1) * sizeof(int), hipHostMallocMapped));
    memset(e->status, 0, 2 * (eftb_engine::NSETS + 1) * sizeof(int));
    HIPCHK(hipDeviceSynchronize());  // the zero fills above ran on the null stream, which the engine's non-blocking streams do not wait for
    *out = guard.release();
    return 0;
}

int eftb_set_table(eftb_engine* e, int id, const void* host, size_t nbytes) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e || !host) return fail("eftb_set_table: null argument");
    if (id < 0 || id >= EFTB_T_COUNT) return fail("eftb_set_table: bad table id %d", id);
    const size_t need = need_table_bytes(e->c, id);
    if (need == 0) return fail("eftb_set_table: table %d is not used by this configuration", id);
    if (need != nbytes) return fail("eftb_set_table: table %d expects %zu bytes, got %zu", id, need, nbytes);
    HIPCHK(hipSetDevice(e->c.device));
    if (!e->tab[id]) HIPCHK(own_dev(e->own, &e->tab[id], nbytes));
    else if (e->finalized) HIPCHK(sync_all(e));  // replacing a resident table (e.g. the AP fiducial): no run may still be reading it
    HIPCHK(hipMemcpy(e->tab[id], host, nbytes, hipMemcpyHostToDevice));
    e->tab_bytes[id] = nbytes;
    if (id == EFTB_T_S) {
        std::vector<double> v(NS);
        const double* sv = static_cast<const double*>(host);
        for (int i = 0; i < NS; ++i) v[i] = 1.0 / (sv[i] * sv[i]);
        HIPCHK(hipMemcpy(e->sm2, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
        for (int i = 0; i < NS; ++i) v[i] = 1.0 / (sv[i] * sv[i] * sv[i] * sv[i]);
        HIPCHK(hipMemcpy(e->sm4, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return 0;
}

int eftb_finalize(eftb_engine* e) {
    if (e) sub_drain(e);
    if (!e) return fail("eftb_finalize: null engine");
    for (int id = 0; id < EFTB_T_COUNT; ++id)
        if (need_table_bytes(e->c, id) && !e->tab[id]) return fail("eftb_finalize: table %d was never set", id);
    HIPCHK(hipSetDevice(e->c.device));
    const eftb_config& c = e->c;
    if (c.with_resum) {
        // split the s sum when the batch alone cannot fill the chip (deterministic two-pass reduction)
        e->resum_splits = c.max_batch >= 16 ? 1 : 8;
        {
            const size_t pbytes = (size_t)c.max_batch * e->resum_splits * 2 * c.Nl * c.Nl * 21 * c.Nk * sizeof(double);
            HIPCHK(own_dev(e->own, &e->part, pbytes, true));  // (zero: the matrix-core kernel never touches k < Nklow)
        }
        if (c.optiresum) HIPCHK(own_dev(e->own, &e->XB, (size_t)c.max_batch * c.Nl * 14 * NS * sizeof(double)));
        if (c.with_nnlo) {
            HIPCHK(own_dev(e->own, &e->ZC, e->buf_elems[EFTB_B_C11] * sizeof(double)));
            HIPCHK(own_dev(e->own, &e->ZC2, e->buf_elems[EFTB_B_CLOOPL] * sizeof(double)));
            HIPCHK(hipMemset(e->ZC, 0, e->buf_elems[EFTB_B_C11] * sizeof(double)));
            HIPCHK(hipMemset(e->ZC2, 0, e->buf_elems[EFTB_B_CLOOPL] * sizeof(double)));
        }
        {
            const size_t abytes = (size_t)c.max_batch * RS_ROWS * RS_NB * sizeof(double);
            HIPCHK(own_dev(e->own, &e->RSA, abytes));
            HIPCHK(own_dev(e->own, &e->RSC, ((size_t)c.max_batch * NS + RS_PF) * RS_REC * sizeof(double)));
            HIPCHK(own_dev(e->own, &e->RSA2, abytes));
            if (c.Nl == 3) {  // one operand per s
                HIPCHK(own_dev(e->own, &e->RSAS, ((size_t)c.max_batch * NS + RS_PF) * RS3_AS * sizeof(double)));
                HIPCHK(own_dev(e->own, &e->RSAS2, ((size_t)c.max_batch * NS + RS_PF) * RS3_AS * sizeof(double)));
            }
            HIPCHK(own_dev(e->own, &e->RSC2, ((size_t)c.max_batch * NS + RS_PF) * RS_REC * sizeof(double)));
        }
    }
    // opt in to the large dynamic LDS tiles
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (c.with_ap) {
        // (the kernel also holds a few static words: the dynamic part must leave room for them below the 160 KB of a CU)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_weights_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_weights_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        {   // which form of the AP stage (see engine.ap_mode): needs the k grid, so it is decided here
            std::vector<double> kh(c.Nk);
            HIPCHK(hipMemcpy(kh.data(), tb<double>(e, EFTB_T_K), c.Nk * sizeof(double), hipMemcpyDeviceToHost));
            const double dk = kh[c.Nk - 1] - kh[c.Nk - 2];
            e->ap_mode = dk > 0.0 && 0.02 * kh[c.Nk - 1] / dk > APW_DCAP / 2 ? 1 : 0;
            if (const char* f = getenv("EFTB_AP_MODE")) e->ap_mode = atoi(f);
            {   // the all-in-LDS form of the direct-P_l AP stage, where its tables fit
                const size_t lds = ((size_t)((c.Nk + 1) & ~1) + (size_t)c.nmu * 8 + 36 * 16 + (size_t)(c.nmu + 1) * 36 + (size_t)(c.Nk - 1) * 12) * sizeof(double);
                e->ap_plk_fused = c.Nl == 3 && lds <= 150 * 1024 && c.nmu >= 2 && c.nmu <= 7 * 32 && !(getenv("EFTB_AP_PLK_FUSED") && !atoi(getenv("EFTB_AP_PLK_FUSED")));
                if (e->ap_plk_fused)
                    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_plk_fused_kernel<3, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            }
#define APM_LDS(NLV, NRV) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_moments_kernel<NLV, NRV, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256))
            APM_LDS(3, 21); APM_LDS(3, NROW); APM_LDS(2, 21); APM_LDS(2, NROW);
#undef APM_LDS
        }
    }
    if (c.with_ap && c.Nl == 3 && !e->PLK0)
        HIPCHK(own_dev(e->own, &e->PLK0, e->buf_elems[EFTB_B_PLK] * sizeof(double), true));
    if (e->ap_overlap && !e->T3) HIPCHK(own_dev(e->own, &e->T3, (e->buf_elems[EFTB_B_TEMPL] + 2) * sizeof(double)));  // third template block (engine.back)
    if (e->ap_overlap && e->c.with_nnlo && e->c.with_ap && !e->T3N) {
        HIPCHK(own_dev(e->own, &e->T3N, (e->buf_elems[EFTB_B_TEMPLN] + 2) * sizeof(double)));
        HIPCHK(own_dev(e->own, &e->TaltN, (e->buf_elems[EFTB_B_TEMPLN] + 2) * sizeof(double)));
        HIPCHK(hipMemset(e->T3N, 0, e->buf_elems[EFTB_B_TEMPLN] * sizeof(double)));
        HIPCHK(hipMemset(e->TaltN, 0, e->buf_elems[EFTB_B_TEMPLN] * sizeof(double)));
    }
    HIPCHK(hipDeviceSynchronize());  // null-stream zero fills (part, ZC, ZC2) are not ordered against the engine's non-blocking streams
    e->finalized = true;
    return 0;
}

int eftb_add_operator(eftb_engine* e, int nl_out, int nx_out, int nl_in, int nx_in, const double* op, int* op_id) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e || !op || !op_id) return fail("eftb_add_operator: null argument");
    if (nl_out < 1 || nx_out < 1 || nl_in < 1 || nx_in < 1) return fail("eftb_add_operator: bad shape");
    if ((size_t)nl_out * nx_out > (size_t)e->c.Nl * e->c.Nk || (size_t)nl_in * nx_in > (size_t)e->c.Nl * e->c.Nk)
        return fail("eftb_add_operator: operator shapes must not exceed the engine's [Nl=%d][Nk=%d] block", e->c.Nl, e->c.Nk);
    HIPCHK(hipSetDevice(e->c.device));
    eftb_engine::Op o{nl_out, nx_out, nl_in, nx_in, (nl_out * nx_out + 15) / 16 * 16, nullptr, -1};
    // K-major copy: opT[(l,k)][(a,x)]
    std::vector<double> t((size_t)nl_in * nx_in * o.ld, 0.0);
    for (int a = 0; a < nl_out; ++a)
        for (int l = 0; l < nl_in; ++l)
            for (int x = 0; x < nx_out; ++x) {
                const double* src = op + (((size_t)a * nl_in + l) * nx_out + x) * nx_in;
                for (int k = 0; k < nx_in; ++k) t[((size_t)l * nx_in + k) * o.ld + (size_t)a * nx_out + x] = src[k];
            }
    HIPCHK(own_dev(e->own, &o.dev, t.size() * sizeof(double)));
    if (int rc = [&] { HIPCHK(hipMemcpy(o.dev, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice)); return 0; }()) {
        e->own.release(o.dev);  // (the operator is not registered: nobody would use the matrix)
        return rc;
    }
    e->ops.push_back(o);
    *op_id = (int)e->ops.size() - 1;
    return 0;
}

int eftb_set_operator_stochastic(eftb_engine* e, int op_id, int st_op_id) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_operator_stochastic: null engine");
    const int n = (int)e->ops.size();
    if (op_id < 0 || op_id >= n || st_op_id < -1 || st_op_id >= n) return fail("eftb_set_operator_stochastic: operator id out of range");
    if (st_op_id >= 0) {
        const eftb_engine::Op &a = e->ops[op_id], &b = e->ops[st_op_id];
        if (a.nl_out != b.nl_out || a.nx_out != b.nx_out || a.nl_in != b.nl_in || a.nx_in != b.nx_in)
            return fail("eftb_set_operator_stochastic: operators %d and %d differ in shape", op_id, st_op_id);
    }
    e->ops[op_id].st_op = st_op_id;
    return 0;
}

int eftb_set_tracers(eftb_engine* e, int ntr) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_tracers: null engine");
    if (ntr < 1 || ntr > e->c.max_batch) return fail("eftb_set_tracers: %d tracers outside [1, max_batch]", ntr);
    e->ntr = ntr;
    ++e->draw_gen;
    e->tracer_ops.clear();
    e->like_ndata = 0;  // a likelihood set for another grouping does not survive
    e->recipe[0].set = e->recipe[1].set = false;  // nor do the draw recipes: their terms name tracers
    e->dset_M = 0;  // nor do the data sets of the groups call: they belong to the likelihood
    ++e->dset_gen;
    return 0;
}

int eftb_set_pipeline_operator_tracer(eftb_engine* e, int tracer, int op_id) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_pipeline_operator_tracer: null engine");
    const int n = (int)e->ops.size();
    if (tracer < 0 || tracer >= e->ntr || op_id < 0 || op_id >= n) return fail("eftb_set_pipeline_operator_tracer: tracer %d / operator %d out of range", tracer, op_id);
    if (e->tracer_ops.empty()) e->tracer_ops.assign(e->ntr, op_id);  // until told otherwise every tracer uses the first one given
    const eftb_engine::Op& b = e->ops[op_id];
    for (int t = 0; t < e->ntr; ++t) {
        const eftb_engine::Op& a = e->ops[e->tracer_ops[t]];
        if (t != tracer && (a.nl_out != b.nl_out || a.nx_out != b.nx_out || a.nl_in != b.nl_in || a.nx_in != b.nx_in))
            return fail("eftb_set_pipeline_operator_tracer: the tracers' operators must share one shape (pad chained outputs with zero rows)");
    }
    e->tracer_ops[tracer] = op_id;
    return 0;
}

int eftb_apply_operator(eftb_engine* e, int op_id, int B) {
    if (e) sub_drain(e);
    if (!e) return fail("eftb_apply_operator: null engine");
    if (!e->finalized) return fail("eftb_apply_operator: engine not finalized");
    if (B < 1 || B > e->c.max_batch) return fail("eftb_apply_operator: batch %d outside [1, %d]", B, e->c.max_batch);
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    ++e->draw_gen;
    if (int rc = launch_operator(e, op_id, B)) return rc;
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(le));
    return 0;
}

int eftb_set_pipeline_operator(eftb_engine* e, int op_id) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_pipeline_operator: null engine");
    if (op_id >= (int)e->ops.size()) return fail("eftb_set_pipeline_operator: operator id %d out of range", op_id);
    e->pipeline_op = op_id < 0 ? -1 : op_id;
    return 0;
}

int eftb_set_template_dims(eftb_engine* e, int nl, int nx) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_template_dims: null engine");
    if (nl < 1 || nx < 1 || (size_t)nl * nx > (size_t)e->c.Nl * e->c.Nk) return fail("eftb_set_template_dims: bad shape [%d][24][%d]", nl, nx);
    e->cur_nl = nl;
    e->cur_nx = nx;
    ++e->draw_gen;
    return 0;
}

int eftb_set_option(eftb_engine* e, int option, int value) {
    if (e && option == EFTB_O_SUBMIT_HOLD) { e->sub_hold.store(value != 0, std::memory_order_release); return 0; }  // (no drain: the queue is meant to stand)
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e) return fail("eftb_set_option: null engine");
    switch (option) {
        case EFTB_O_AP_STOCHASTIC: e->c.ap_stochastic = value ? 1 : 0; return 0;
        case EFTB_O_JEFFREYS: e->jeffreys = value ? 1 : 0; return 0;
        case EFTB_O_GRAPH: e->use_graphs = value != 0; return 0;
        case EFTB_O_CHECK_FINITE: e->check_finite = value != 0; return 0;
        case EFTB_O_TIME_DOMINANT: e->time_dominant = value < 0 ? 0 : value; e->time_seqk[0] = e->time_seqk[1] = e->time_seqk[2] = 0; return 0;
        case EFTB_O_LATENCY_MODE: e->latency_auto = value != 0; return 0;
        case EFTB_O_PLK_DIRECT: e->plk_direct = value != 0; return 0;
        case EFTB_O_STEP_TRACE:
            if (value && !e->evTraceBase) {
                HIPCHK(hipSetDevice(e->c.device));
                HIPCHK(own_event(e->own, &e->evTraceBase));
                for (auto& row : e->evTrace)
                    for (hipEvent_t& ev : row) HIPCHK(own_event(e->own, &ev));
            }
            if (value) {
                HIPCHK(hipEventRecord(e->evTraceBase, e->stream));
                e->trace_n = 0;
            }
            e->trace_on = value != 0;
            return 0;
        case EFTB_O_SUBMIT_HOLD: e->sub_hold.store(value != 0, std::memory_order_release); return 0;
        case EFTB_O_SUBMIT_THREAD:
            if (value < 0 || value > 2) return fail("eftb_set_option: EFTB_O_SUBMIT_THREAD takes 0, 1 or 2");
            e->sub_mode = value; return 0;
        case EFTB_O_TIME_KERNEL:
            if (value < 1 || value > 7) return fail("eftb_set_option: EFTB_O_TIME_KERNEL takes a set of 1 (resummation) | 2 (synthesis) | 4 (AP knot weights)");
            e->time_kernel = value; return 0;
    }
    return fail("eftb_set_option: unknown option %d", option);
}

int eftb_dominant_time(eftb_engine* e, double* ms_sum, long long* launches, int reset) {
    if (e) sub_drain(e);
    if (!e || !ms_sum || !launches) return fail("eftb_dominant_time: null argument");
    HIPCHK(hipSetDevice(e->c.device));
    return eftb_kernel_time(e, 0, ms_sum, launches, reset);
}

int eftb_kernel_time(eftb_engine* e, int kind, double* ms_sum, long long* launches, int reset) {
    if (e) sub_drain(e);
    if (!e || !ms_sum || !launches) return fail("eftb_kernel_time: null argument");
    if (kind < 0 || kind > 2) return fail("eftb_kernel_time: kind %d (0 resummation, 1 synthesis, 2 AP knot weights)", kind);
    HIPCHK(hipSetDevice(e->c.device));
    collect_timer(e, -1, true);
    *ms_sum = e->timer_ms[kind];
    *launches = e->timer_n[kind];
    if (reset) {
        e->timer_ms[kind] = 0.0;
        e->timer_n[kind] = 0;
        e->timer_cosmo[kind] = 0;
    }
    return 0;
}

int eftb_kernel_time_ex(eftb_engine* e, int kind, double* ms_sum, long long* launches, long long* cosmologies, int reset) {
    if (!cosmologies) return fail("eftb_kernel_time_ex: null argument");
    if (e && kind >= 0 && kind <= 2) {
        sub_drain(e);
        (void)hipSetDevice(e->c.device);
        collect_timer(e, -1, true);
        *cosmologies = e->timer_cosmo[kind];
    }
    return eftb_kernel_time(e, kind, ms_sum, launches, reset);
}

int eftb_set_likelihood(eftb_engine* e, int ndata, const int32_t* index, const double* data, const double* invcov, int nG, const double* mu,
                        const double* sigma_inv) {
    if (e) sub_drain(e);
    if (e) ++e->epoch;  // invalidates the captured graphs
    if (!e || !index || !data || !invcov || (nG > 0 && (!mu || !sigma_inv))) return fail("eftb_set_likelihood: null argument");
    if (nG < 0 || nG > MARG_MAXG) return fail("eftb_set_likelihood: nG=%d outside [0, %d]", nG, MARG_MAXG);  // nG = 0: plain -chi2 / 2
    if (ndata < 1) return fail("eftb_set_likelihood: ndata=%d", ndata);
    // the shape the index refers to: what the PROJECT stage will produce if an operator is registered for it and the block has not been
    // projected yet, else the block as it is; the LOGP stage checks it again at launch
    int lnl = e->cur_nl, lnx = e->cur_nx;
    {
        const int op = !e->tracer_ops.empty() ? e->tracer_ops[0] : e->pipeline_op;
        if (op >= 0 && e->ops[op].nl_in == e->cur_nl && e->ops[op].nx_in == e->cur_nx) {
            lnl = e->ops[op].nl_out;
            lnx = e->ops[op].nx_out;
        }
    }
    const int npts = e->ntr * lnl * lnx;  // the walker's ntr entries are addressed as one block of ntr * nl multipoles
    for (int a = 0; a < ndata; ++a)
        if (index[a] < 0 || index[a] >= npts)
            return fail("eftb_set_likelihood: index[%d]=%d outside the template block [%d x %d][24][%d]", a, index[a], e->ntr, lnl, lnx);
    for (int a = 0; a < ndata; ++a)
        for (int b2 = 0; b2 < a; ++b2) {
            // symmetric up to the rounding of a matrix inversion (the reference passes np.linalg.inv(cov) as it comes out, likelihood.py:372):
            // measured against the diagonal, not against the element itself -- small off-diagonal entries carry the inversion's absolute error
            const double x = invcov[(size_t)a * ndata + b2], y = invcov[(size_t)b2 * ndata + a];
            const double sc = sqrt(fabs(invcov[(size_t)a * ndata + a] * invcov[(size_t)b2 * ndata + b2]));
            if (fabs(x - y) > 1e-8 * sc + 1e-300) return fail("eftb_set_likelihood: invcov is not symmetric at (%d, %d)", a, b2);
        }
    HIPCHK(hipSetDevice(e->c.device));
    HIPCHK(sync_all(e));  // a likelihood stage of an overlapped run may still be reading the old tables on the back-half stream
    drop_likelihood(e);
    {
        const size_t vb = (size_t)(e->c.max_batch / e->ntr + 1) * (nG + 1) * ndata * sizeof(double);
        HIPCHK(own_dev(e->own, &e->like_V, vb));
        HIPCHK(own_dev(e->own, &e->like_U, vb));
    }
    HIPCHK(own_dev(e->own, &e->like_index, ndata * sizeof(int)));
    HIPCHK(own_dev(e->own, &e->like_data, ndata * sizeof(double)));
    HIPCHK(own_dev(e->own, &e->like_invcov, (size_t)ndata * ndata * sizeof(double)));
    HIPCHK(own_dev(e->own, &e->like_mu, MARG_MAXG * sizeof(double)));
    HIPCHK(own_dev(e->own, &e->like_sinv, MARG_MAXG * sizeof(double)));
    HIPCHK(hipMemcpy(e->like_index, index, ndata * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->like_data, data, ndata * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->like_invcov, invcov, (size_t)ndata * ndata * sizeof(double), hipMemcpyHostToDevice));
    if (nG > 0) {
        HIPCHK(hipMemcpy(e->like_mu, mu, nG * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->like_sinv, sigma_inv, nG * sizeof(double), hipMemcpyHostToDevice));
    }
    e->like_ndata = ndata;
    e->like_nG = nG;
    e->like_nl = lnl;
    e->like_nx = lnx;
    e->recipe[0].set = false;  // the logp recipe belongs to the likelihood it was set for
    e->dset_M = 0;  // and so do the data sets (eftb_set_likelihood_datasets)
    ++e->dset_gen;
    ++e->draw_gen;
    return 0;
}

void eftb_destroy(eftb_engine* e) {
    if (!e) return;
    sub_stop_thread(e);
    (void)hipSetDevice(e->c.device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (hipStream_t q : {e->pre, e->side, e->cpy, e->back}) if (q) (void)hipStreamSynchronize(q);  // look-ahead work and staged uploads still in flight
    drop_graphs(e);
    if (e->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm);
    if (e->sub_stats && e->issue_n)
        fprintf(stderr, "[eftbird] staged steps: %llu issued (%llu by the caller's thread), %.1f us per step in the issuing thread, %.1f us filling the staging block, "
                        "%.1f us waiting for results\n", e->issue_n, e->inline_n, e->issue_ns / e->issue_n * 1e-3, e->fill_ns / e->issue_n * 1e-3, e->wait_ns / e->issue_n * 1e-3);
    delete e;  // the ledger releases what the engine holds, newest first: memory and events before the streams they were used on
}

size_t eftb_buffer_size(const eftb_engine* e, int id) {
    if (!e || id < 0 || id >= EFTB_B_COUNT) return 0;
    return e->buf_elems[id];
}

int eftb_put(eftb_engine* e, int id, size_t offset, const double* host, size_t count) {
    if (e) sub_drain(e);
    if (!e || !host) return fail("eftb_put: null argument");
    if (id < 0 || id >= EFTB_B_COUNT || !e->buf[id]) return fail("eftb_put: buffer %d not available in this configuration", id);
    if (offset + count > e->buf_elems[id]) return fail("eftb_put: buffer %d holds %zu elements, asked [%zu, %zu)", id, e->buf_elems[id], offset, offset + count);
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    HIPCHK(hipMemcpyAsync(e->buf[id] + offset, host, count * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (id == EFTB_B_TEMPL || id == EFTB_B_TEMPLN) {
        ++e->draw_gen;
        if (id == EFTB_B_TEMPL) {  // (the block holds templates again; what the caller wrote starts at 0 or continues what is there)
            e->templ_elems = offset == 0 || !e->templ_ok ? offset + count : std::max(e->templ_elems, offset + count);
            e->templ_ok = true;
        }
    }
    return 0;
}

int eftb_get(eftb_engine* e, int id, size_t offset, double* host, size_t count) {
    if (e) sub_drain(e);
    if (!e || !host) return fail("eftb_get: null argument");
    if (id < 0 || id >= EFTB_B_COUNT || !e->buf[id]) return fail("eftb_get: buffer %d not available in this configuration", id);
    if (offset + count > e->buf_elems[id]) return fail("eftb_get: buffer %d holds %zu elements, asked [%zu, %zu)", id, e->buf_elems[id], offset, offset + count);
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    HIPCHK(hipMemcpyAsync(host, e->buf[id] + offset, count * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_status(e, "eftb_get");
}

int eftb_run(eftb_engine* e, int mask, int B) {
    if (e) sub_drain(e);
    if (!e) return fail("eftb_run: null engine");
    if (!e->finalized) return fail("eftb_run: engine not finalized");
    if (B < 1 || B > e->c.max_batch) return fail("eftb_run: batch %d outside [1, %d]", B, e->c.max_batch);
    HIPCHK(hipSetDevice(e->c.device));
    const int slot = (int)(e->run_seq % eftb_engine::RUN_DEPTH);
    if (e->run_seq >= eftb_engine::RUN_DEPTH)  // the run launched RUN_DEPTH calls ago must have finished (spin: it almost always has)
        if (int rc = spin_event(e->evRun[slot], "eftb_run", "the run launched RUN_DEPTH calls ago")) return rc;
    e->status_slot = eftb_engine::NSETS;
    e->inputs_settled = true;  // eftb_put is synchronous: the inputs of this run are in place, its first stage may start early
    e->allow_back = true;
    e->run_direct = false;
    const int rc = run_stages(e, mask, B);
    e->inputs_settled = e->allow_back = false;
    if (rc) return rc;
    note_templates(e, mask, B);
    HIPCHK(hipEventRecord(e->evRun[slot], e->back_pending ? e->back : e->stream));  // the run ends where its back half ran
    ++e->run_seq;
    return 0;
}

int eftb_sync(eftb_engine* e) {
    if (e) sub_drain(e);
    if (!e) return fail("eftb_sync: null engine");
    join_back(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_status(e, "eftb_sync");
}

int eftb_run_timed(eftb_engine* e, int mask, int B, int repeats, float* ms) {
    if (e) sub_drain(e);
    if (!e || !ms) return fail("eftb_run_timed: null argument");
    if (!e->finalized) return fail("eftb_run_timed: engine not finalized");
    if (B < 1 || B > e->c.max_batch) return fail("eftb_run_timed: batch %d outside [1, %d]", B, e->c.max_batch);
    if (repeats < 1) repeats = 1;
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    e->run_direct = false;
    for (int r = 0; r < repeats; ++r)
        if (int rc = launch_stages(e, mask, B)) return rc;
    note_templates(e, mask, B);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    HIPCHK(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return 0;
}

// inputs of one batch -> device (engine stream), then the theory stages of reference theory.py:557-585
static int upload_and_launch(eftb_engine* e, const char* who, int B, const double* Pin, const double* f, const double* DA, const double* H,
                             int extra_mask) {
    if (!e->finalized) return fail("%s: engine not finalized", who);
    const eftb_config& c = e->c;
    if (B < 1 || B > c.max_batch) return fail("%s: batch %d outside [1, %d]", who, B, c.max_batch);
    if (c.with_ap && (!DA || !H)) return fail("%s: DA and H are required when with_ap=1", who);
    if (int rc = validate_inputs(c, who, B, Pin, f, DA, H)) return rc;
    HIPCHK(hipSetDevice(c.device));
    join_back(e);
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(e->buf[EFTB_B_PIN], Pin, (size_t)B * c.Nkin * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->buf[EFTB_B_F], f, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    if (c.with_ap) {
        HIPCHK(hipMemcpyAsync(e->buf[EFTB_B_DA], DA, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->buf[EFTB_B_H], H, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    }
    int mask = EFTB_S_PREP | EFTB_S_LOOPS | EFTB_S_REGROUP | extra_mask;
    if (c.with_resum) mask |= EFTB_S_CF | EFTB_S_RESUM;
    if (c.with_ap) mask |= EFTB_S_AP;
    if (e->pipeline_op >= 0 || !e->tracer_ops.empty()) mask |= EFTB_S_PROJECT;
    e->run_direct = false;
    if (int rc = run_stages(e, mask, B)) return rc;
    note_templates(e, mask, B);
    return 0;
}

int eftb_eval_batch(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA, const double* H, double* templ,
                    const double* bias, double* plk) {
    if (e) sub_drain(e);
    if (!e || !Pin || !f || (!templ && !plk)) return fail("eftb_eval_batch: null argument");
    if (plk && !bias) return fail("eftb_eval_batch: bias is required when plk is requested");
    if (plk && B >= 1 && B <= e->c.max_batch) {
        HIPCHK(hipSetDevice(e->c.device));
        join_back(e);  // a back half still in flight (reduce / likelihood of an asynchronous eftb_run) reads BIAS
        HIPCHK(hipMemcpyAsync(e->buf[EFTB_B_BIAS], bias, (size_t)B * NROW * sizeof(double), hipMemcpyHostToDevice, e->stream));
    }
    if (int rc = upload_and_launch(e, "eftb_eval_batch", B, Pin, f, DA, H, plk ? EFTB_S_REDUCE : 0)) return rc;
    hipStream_t st = e->stream;
    if (templ)
        HIPCHK(hipMemcpyAsync(templ, e->buf[EFTB_B_TEMPL], (size_t)B * e->cur_nl * NROW * e->cur_nx * sizeof(double), hipMemcpyDeviceToHost, st));
    if (plk) HIPCHK(hipMemcpyAsync(plk, e->buf[EFTB_B_PLK], (size_t)B * e->cur_nl * e->cur_nx * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return check_status(e, "eftb_eval_batch");
}

int eftb_eval_logp_batch(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA, const double* H, const double* rows,
                         double* logp, double* fullchi2, double* best) {
    if (e) sub_drain(e);
    if (!e || !Pin || !f || !rows || !logp) return fail("eftb_eval_logp_batch: null argument");
    if (!e->finalized) return fail("eftb_eval_logp_batch: engine not finalized");
    if (!e->like_ndata) return fail("eftb_eval_logp_batch: needs eftb_set_likelihood");
    if (B < 1 || B > e->c.max_batch) return fail("eftb_eval_logp_batch: batch %d outside [1, %d]", B, e->c.max_batch);
    HIPCHK(hipSetDevice(e->c.device));
    hipStream_t st = e->stream;
    const int ng1 = e->like_nG + 1;
    join_back(e);  // a back half still in flight reads GROWS
    // rows arrive packed [B][nG+1][24]; the device block is [B][MARG_NG1][24]
    HIPCHK(hipMemcpy2DAsync(e->buf[EFTB_B_GROWS], (size_t)MARG_NG1 * NROW * sizeof(double), rows, (size_t)ng1 * NROW * sizeof(double),
                            (size_t)ng1 * NROW * sizeof(double), B, hipMemcpyHostToDevice, st));
    if (int rc = upload_and_launch(e, "eftb_eval_logp_batch", B, Pin, f, DA, H, EFTB_S_LOGP)) return rc;
    const int nw = B / e->ntr;  // one result per likelihood point
    e->like_host.resize((size_t)nw * MARG_OUT);
    HIPCHK(hipMemcpyAsync(e->like_host.data(), e->buf[EFTB_B_LOGP], (size_t)nw * MARG_OUT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = check_status(e, "eftb_eval_logp_batch")) return rc;
    for (int w = 0; w < nw; ++w) {
        const double* o = e->like_host.data() + (size_t)w * MARG_OUT;
        logp[w] = o[0];
        if (fullchi2) fullchi2[w] = o[1];
        if (best)
            for (int i = 0; i < e->like_nG; ++i) best[(size_t)w * e->like_nG + i] = o[2 + i];
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ parameter draws (fast / slow split)
// device buffer of at least n elements: grows, never shrinks (held by the engine's ledger); separate from every buffer of the runs.  With
// who, a failed allocation is that call's refusal and names what, of which shape, asked for it; without, it fails as every HIP call does
static int grow_dev(eftb_engine* e, void* pp, size_t* cap, size_t n, size_t elem = sizeof(double), const char* who = nullptr, const char* what = nullptr,
                    const char* shape = nullptr) {
    void** p = static_cast<void**>(pp);
    if (n <= *cap) return 0;
    e->own.release(*p);
    *cap = 0;
    if (!who) HIPCHK(own_dev(e->own, p, n * elem));
    else if (hipError_t me = own_dev(e->own, p, n * elem); me != hipSuccess) {
        (void)hipGetLastError();
        return fail("%s: no device memory for %s of %s (%zu bytes): %s", who, what, shape, n * elem, hipGetErrorString(me));
    }
    *cap = n;
    return 0;
}

static int launched(const char* who) {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : fail("%s: kernel launch failed: %s", who, hipGetErrorString(le));
}

// offsets (walker c owns draws [offsets[c], offsets[c + 1])) and the state of the template block; *maxcnt: the most draws one walker owns.
// A groups call (eftb_draws_logp_params_datasets) passes its G groups as C, unit = "group" and nwalk, the walkers the block must hold
static int draws_check(eftb_engine* e, const char* who, int C, long long N, const int64_t* offsets, long long* maxcnt, const char* unit = "walker",
                       int nwalk = -1) {
    if (!e->finalized) return fail("%s: engine not finalized", who);
    if (C < 1) return fail("%s: %d %ss", who, C, unit);
    if (N < 0) return fail("%s: %lld draws", who, N);
    if (offsets[0] != 0) return fail("%s: offsets[0] = %lld, not 0", who, (long long)offsets[0]);
    long long mx = 0;
    for (int w = 0; w < C; ++w) {
        if (offsets[w + 1] < offsets[w]) return fail("%s: offsets decrease at %s %d (%lld -> %lld)", who, unit, w, (long long)offsets[w], (long long)offsets[w + 1]);
        mx = std::max<long long>(mx, offsets[w + 1] - offsets[w]);
    }
    if (offsets[C] != N) return fail("%s: offsets[%d] = %lld, not the %lld draws", who, C, (long long)offsets[C], N);
    if (!e->templ_ok)
        return fail("%s: the current block holds no templates (the last run was a direct-P_l run, or a staged step has rotated the blocks since the "
                    "last template-producing run / eftb_put)", who);
    const size_t per = (size_t)e->cur_nl * NROW * e->cur_nx, have = per ? e->templ_elems / per : 0;
    if (nwalk < 0) nwalk = C;
    if ((size_t)nwalk * e->ntr > have)
        return fail("%s: %d walkers x %d tracers, but the template block holds %zu entries [%d][24][%d]", who, nwalk, e->ntr, have, e->cur_nl, e->cur_nx);
    *maxcnt = mx;
    return 0;
}

// workgroups per walker: enough for its draws (per_wg at a time), about 2048 in all
static int draw_shares(long long maxcnt, int per_wg, long long groups) {
    const long long want = (maxcnt + per_wg - 1) / per_wg, fill = std::max(1LL, 2048 / std::max(1LL, groups));
    return (int)std::max(1LL, std::min(want, fill));
}

// W_c [C][J1][J1] of the current block, likelihood and tracers: built when the cached block is of another generation or holds fewer walkers
static int draws_gram(eftb_engine* e, const char* who, int C, int J1) {
    const eftb_config& c = e->c;
    const int ntr = e->ntr, nd = e->like_ndata;
    hipStream_t st = e->stream;
    if (e->gram_gen != e->draw_gen || e->gram_C < C) {
        e->gram_gen = 0;
        const size_t ae = (size_t)C * J1 * nd;
        if (int rc = grow_dev(e, &e->drw_A, &e->drw_A_cap, ae)) return rc;
        if (int rc = grow_dev(e, &e->drw_U, &e->drw_U_cap, ae)) return rc;
        if (int rc = grow_dev(e, &e->drw_W, &e->drw_W_cap, (size_t)C * J1 * J1)) return rc;
        hipLaunchKernelGGL(draws_gather_kernel, dim3(C), dim3(256), 0, st, e->cur_nl, e->cur_nx, ntr, nd, J1, e->like_index, e->like_data,
                           e->buf[EFTB_B_TEMPL], c.with_nnlo ? e->buf[EFTB_B_TEMPLN] : nullptr, e->drw_A);
        launch_times_invcov(e, st, e->drw_A, C * J1, e->drw_U);  // U = A C^-1 for all walkers, exactly as the LOGP stage multiplies V
        const int gy = std::min(1024, (J1 * J1 + 63) / 64);
        hipLaunchKernelGGL(draws_gram_kernel, dim3(C, gy), dim3(256), 0, st, nd, J1, e->drw_A, e->drw_U, e->drw_W);
        if (int rc = launched(who)) return rc;
        e->gram_gen = e->draw_gen;
        e->gram_C = C;
    }
    return 0;
}

// a [MARG_OUT] record of a logp draw kernel -> slot `to` of logp, fullchi2 and best [..][nG], where the caller asks for them
static void draws_unpack(const double* o, int nG, size_t to, double* logp, double* fullchi2, double* best) {
    if (logp) logp[to] = o[0];
    if (fullchi2) fullchi2[to] = o[1];
    if (best) std::copy_n(o + 2, nG, best + to * nG);
}

// the [N][MARG_OUT] records of a logp draw kernel -> logp [N], fullchi2 [N], best [N][nG] (synchronises the stream)
static int draws_records(eftb_engine* e, long long N, double* logp, double* fullchi2, double* best) {
    hipStream_t st = e->stream;
    e->drw_host.resize((size_t)N * MARG_OUT);
    HIPCHK(hipMemcpyAsync(e->drw_host.data(), e->drw_out, (size_t)N * MARG_OUT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (long long d = 0; d < N; ++d) draws_unpack(e->drw_host.data() + (size_t)d * MARG_OUT, e->like_nG, (size_t)d, logp, fullchi2, best);
    return 0;
}

// what every logp draw call refuses before it looks at its own inputs: no likelihood, draws_check, a block of another shape than the likelihood's
static int draws_logp_check(eftb_engine* e, const char* who, int C, long long N, const int64_t* offsets, long long* maxcnt, const char* unit = "walker",
                            int nwalk = -1) {
    if (!e->like_ndata) return fail("%s: needs eftb_set_likelihood", who);
    if (int rc = draws_check(e, who, C, N, offsets, maxcnt, unit, nwalk)) return rc;
    if (e->cur_nl != e->like_nl || e->cur_nx != e->like_nx)
        return fail("%s: the likelihood's data index addresses templates [%d][24][%d], the block is [%d][24][%d]", who, e->like_nl, e->like_nx, e->cur_nl,
                    e->cur_nx);
    return 0;
}

// workgroup of a logp draw kernel of one kind (with the recipe rcp, unless rows): J1 columns of W_c, its LDS layout, nw waves (as many as the
// LDS holds beside W_c; 0: not even one, which the caller words) and the launch's lds bytes
struct DrawShape {
    int J1, nw;
    DrawLds L;
    size_t lds;
};
static int draws_logp_shape(eftb_engine* e, const char* who, DrawKind kind, const eftb_engine::Recipe* rcp, DrawShape* sh) {
    const int J1 = (e->c.with_nnlo ? NROW + 3 : NROW) * e->ntr + 1;
    if (J1 > DRAW_MAXJ1) return fail("%s: %d template columns per walker, at most %d", who, J1 - 1, DRAW_MAXJ1 - 1);
    const DrawLds L = DrawLds::of(kind, J1, e->like_nG, rcp ? rcp->nnz : 0, rcp ? rcp->ndt : 0, rcp ? rcp->P : 0, e->jeffreys);
    const int nw = L.fit(160 * 1024);
    *sh = DrawShape{J1, nw, L, L.bytes(nw)};
    return 0;
}

// Reachable from the sample call alone (which words it anew): J + 1 <= 121 (five tracers; with NNLO four, 109), nG <= 24 and at most
// 1024 recipe entries leave the rows, params, gradient and chain calls at most 146328, 159336, 163432 and 161288 of the 163840 bytes at
// one wave, so this message is never seen.
static int draws_no_fit(const char* who, int J1) { return fail("%s: the Gram matrix of %d columns does not fit the LDS", who, J1); }

// draws_temper_params_kernel is named at the end of this file alone: a kernel is emitted where it is first named, and behind every other one
// it leaves their compiled code, label numbers included, the parent's (isa_counts.json)
using TemperKernel = decltype(&draws_temper_params_kernel<false>);
static TemperKernel temper_kernel(bool two);
// (and draws_ensemble_params_kernel behind it, for the same reason)
using EnsembleKernel = decltype(&draws_ensemble_params_kernel<false>);
static EnsembleKernel ensemble_kernel(bool two);

// the large dynamic LDS for every logp draw kernel, once per engine
static int draws_lds_optin(eftb_engine* e) {
    if (e->drw_lds) return 0;
#define DRAW_PAIR(k) reinterpret_cast<const void*>(&k<false>), reinterpret_cast<const void*>(&k<true>)
    for (const void* k : {DRAW_PAIR(draws_logp_kernel), DRAW_PAIR(draws_logp_params_kernel), DRAW_PAIR(draws_logp_grad_params_kernel),
                          DRAW_PAIR(draws_logp_hess_params_kernel), DRAW_PAIR(draws_sample_params_kernel), DRAW_PAIR(draws_chain_params_kernel),
                          reinterpret_cast<const void*>(temper_kernel(false)), reinterpret_cast<const void*>(temper_kernel(true)),
                          reinterpret_cast<const void*>(ensemble_kernel(false)), reinterpret_cast<const void*>(ensemble_kernel(true))})
        HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#undef DRAW_PAIR
    e->drw_lds = true;
    return 0;
}

// before the inputs of a logp draw call go to the device: the device and the stream, the LDS opt-in of the kernels (once), W_c, the
// record buffer, and the offsets (a groups call: C groups own the draws, W_c is wanted for nwalk walkers)
static int draws_logp_begin(eftb_engine* e, const char* who, int C, long long N, int J1, const int64_t* offsets, int nwalk = -1) {
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    if (int rc = draws_lds_optin(e)) return rc;
    if (int rc = draws_gram(e, who, nwalk < 0 ? C : nwalk, J1)) return rc;
    if (int rc = grow_dev(e, &e->drw_off, &e->drw_off_cap, (size_t)C + 1, sizeof(long long))) return rc;
    if (int rc = grow_dev(e, &e->drw_out, &e->drw_out_cap, (size_t)N * MARG_OUT)) return rc;
    HIPCHK(hipMemcpyAsync(e->drw_off, offsets, ((size_t)C + 1) * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    return 0;
}

int eftb_draws_logp(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* rows, const double* rows_nnlo, double* logp,
                    double* fullchi2, double* best) {
    static const char* who = "eftb_draws_logp";
    if (e) sub_drain(e);
    if (!e || !offsets || (N > 0 && (!rows || !logp))) return fail("%s: null argument", who);
    long long maxcnt = 0;
    if (int rc = draws_logp_check(e, who, C, N, offsets, &maxcnt)) return rc;
    if (rows_nnlo && !e->c.with_nnlo) return fail("%s: rows_nnlo needs an engine built with with_nnlo", who);
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_ROWS, nullptr, &sh)) return rc;
    if (!sh.nw) return draws_no_fit(who, sh.J1);
    if (N == 0) return 0;
    if (int rc = draws_logp_begin(e, who, C, N, sh.J1, offsets)) return rc;
    const int ntr = e->ntr, nG = e->like_nG, ng1 = nG + 1, J1 = sh.J1;
    hipStream_t st = e->stream;
    const size_t rn = (size_t)N * ntr * ng1 * NROW, rnn = (size_t)N * ntr * ng1 * 3;
    if (int rc = grow_dev(e, &e->drw_in, &e->drw_in_cap, rn)) return rc;
    if (rows_nnlo)
        if (int rc = grow_dev(e, &e->drw_inn, &e->drw_inn_cap, rnn)) return rc;
    HIPCHK(hipMemcpyAsync(e->drw_in, rows, rn * sizeof(double), hipMemcpyHostToDevice, st));
    if (rows_nnlo) HIPCHK(hipMemcpyAsync(e->drw_inn, rows_nnlo, rnn * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid(C, draw_shares(maxcnt, sh.nw, C)), block(64 * sh.nw);
    launch_two(draws_logp_kernel<false>, draws_logp_kernel<true>, sh.J1, grid, block, sh.lds, st, ntr, nG, J1, e->jeffreys, e->drw_off, e->drw_in,
               rows_nnlo ? e->drw_inn : nullptr, e->drw_W, e->like_mu, e->like_sinv, e->drw_out);
    if (int rc = launched(who)) return rc;
    return draws_records(e, N, logp, fullchi2, best);
}

void* eftb_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail("eftb_host_alloc: hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void eftb_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

static const int kStagedIds[] = {EFTB_B_PIN, EFTB_B_F, EFTB_B_DA, EFTB_B_H, EFTB_B_BIAS, EFTB_B_GROWS, EFTB_B_PLK, EFTB_B_LOGP};

static const int kStagedIn[] = {EFTB_B_PIN, EFTB_B_F, EFTB_B_DA, EFTB_B_H, EFTB_B_BIAS, EFTB_B_GROWS};  // order inside a set's input block
static const int kStagedOut[] = {EFTB_B_PLK, EFTB_B_LOGP};

// the environment switches of the staged path, read once, when the first step is staged; sb: cosmologies a step brings at most
static void read_staged_switches(eftb_engine* e, size_t sb) {
    if (const char* f = getenv("EFTB_LATENCY_MODE")) e->latency_auto = atoi(f) != 0;
    if (const char* f = getenv("EFTB_DONE_WORDS")) e->done_words = atoi(f) != 0;
    if (const char* f = getenv("EFTB_PLK_DMA")) e->plk_dma = atoi(f) != 0;
    if (const char* f = getenv("EFTB_SUB_STATS")) e->sub_stats = atoi(f) != 0;
    if (const char* f = getenv("EFTB_SUB_INFLIGHT")) e->sub_inflight = std::max(1, std::min(eftb_engine::NSETS - 1, atoi(f)));
    if (const char* f = getenv("EFTB_SUB_LOW")) e->sub_low = std::max(1, atoi(f));
    e->sub_low = std::min(e->sub_low, e->sub_inflight);
    e->coalesce_max = e->comm ? 1 : (int)std::min<size_t>(MAX_COALESCE, (size_t)e->c.max_batch / sb);   // (with a communicator every step is exchanged by itself)
    if (const char* f = getenv("EFTB_COALESCE")) e->coalesce_max = std::max(1, std::min(e->coalesce_max, atoi(f)));
}

// Every set keeps its inputs in ONE device block with the layout of the page-locked staging blocks, so that staging is one upload
// kernel (small separate copies are carried out by the host thread once the stream's dependencies have resolved,
// which would stall the sampler loop for a whole step).
static int staged_acquire(eftb_engine* e) {
    HIPCHK(hipSetDevice(e->c.device));
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (int rc = pad_streams(e, 4, prio_hi)) return rc;
    HIPCHK(own_stream(e->own, &e->cpy, prio_hi));
    size_t off = 0;
    for (int id : kStagedIn) {
        e->stage_off[id] = off;
        off += e->buf_elems[id];
    }
    e->stage_elems = (off + 1) & ~(size_t)1;  // whole double2s for the copy kernel
    for (int id : kStagedIds) e->orig[id] = e->buf[id];
    for (int q = 0; q < eftb_engine::NSETS; ++q) {
        HIPCHK(own_dev(e->own, &e->setblock[q], e->stage_elems * sizeof(double), true));
        for (int id : kStagedIn) e->setbuf[q][id] = e->buf_elems[id] ? e->setblock[q] + e->stage_off[id] : nullptr;
        // per-step outputs: ln P (a few KB) lives in page-locked host memory mapped into the device and is written by the kernel itself;
        // P_l stays in device memory and is copied to page-locked host memory by the DMA engine on the stream the step ends on (the back-half
        // stream in pipelined steps: round 1 measured ~70 us of stalled compute queue per step for such a transfer on the COMPUTE stream)
        for (int id : kStagedOut) {
            if (id == EFTB_B_PLK) {
                HIPCHK(own_dev(e->own, &e->setbuf[q][id], e->buf_elems[id] * sizeof(double), true));
                if (!e->comm) {
                    HIPCHK(own_host(e->own, &e->plk_host[q], e->buf_elems[id] * sizeof(double), hipHostMallocMapped));  // (mapped: latency-mode steps write it from the kernel)
                    memset(e->plk_host[q], 0, e->buf_elems[id] * sizeof(double));
                }
                continue;
            }
            HIPCHK(own_host(e->own, &e->setbuf[q][id], e->buf_elems[id] * sizeof(double), hipHostMallocMapped));
            memset(e->setbuf[q][id], 0, e->buf_elems[id] * sizeof(double));
        }
        HIPCHK(own_event(e->own, &e->evSetDone[q], hipEventDisableTiming));
        HIPCHK(hipEventRecord(e->evSetDone[q], e->cpy));
    }
    // a staging block is sized for one step (step_batch cosmologies), laid out like the device block of a set that holds only that step
    const size_t sb = e->c.step_batch > 0 ? (size_t)e->c.step_batch : (size_t)e->c.max_batch;
    size_t hoff = 0;
    for (int id : kStagedIn) {
        e->slot_off[id] = hoff;
        hoff += e->buf_elems[id] / e->c.max_batch * sb;
    }
    e->slot_elems = (hoff + 1) & ~(size_t)1;
    for (int h = 0; h < eftb_engine::NSLOT; ++h) {
        HIPCHK(own_host(e->own, &e->stage_host[h], e->slot_elems * sizeof(double), hipHostMallocMapped));
        memset(e->stage_host[h], 0, e->slot_elems * sizeof(double));
    }
    for (int r = 0; r < eftb_engine::NLRING; ++r) {
        HIPCHK(own_event(e->own, &e->evStagedR[r], hipEventDisableTiming));
        HIPCHK(own_event(e->own, &e->evStagedAllR[r], hipEventDisableTiming));
        HIPCHK(hipEventRecord(e->evStagedR[r], e->cpy));
        HIPCHK(hipEventRecord(e->evStagedAllR[r], e->cpy));
    }
    read_staged_switches(e, sb);
    {
        void* p = nullptr;
        HIPCHK(own_host(e->own, &p, 2 * eftb_engine::NSETS * sizeof(unsigned long long), hipHostMallocMapped));
        memset(p, 0, 2 * eftb_engine::NSETS * sizeof(unsigned long long));
        e->set_done = static_cast<volatile unsigned long long*>(p);
    }
    e->cur_set = eftb_engine::NSETS - 1;  // the engine's own buffers are current until the first staged launch; sets 0, 1, 2, 3 follow in turn
    HIPCHK(hipDeviceSynchronize());  // the zero fills ran on the null stream; the copy stream is about to write into these blocks
    return 0;
}

// all of it or none: a set-up that failed half way gives back what it got and leaves no copy stream, which every staged entry point looks at --
// the next eftb_stage_inputs starts over, and assigns every field again
static int staged_setup(eftb_engine* e) {
    if (e->cpy) return 0;
    const Ledger::Mark before = e->own.mark();
    const int rc = staged_acquire(e);
    if (rc) {
        e->own.release_to(before);  // (releasing device memory waits for the zero fills in flight, releasing the stream for what was recorded on it)
        e->cpy = nullptr;
    }
    return rc;
}

// ---- staged steps: the host part (inputs -> page-locked block `slot`) ...
static void stage_fill(eftb_engine* e, int slot, int B, const double* Pin, const double* f, const double* DA, const double* H, const double* bias,
                       const double* rows) {
    const eftb_config& c = e->c;
    double* h = e->stage_host[slot];
    memcpy(h + e->slot_off[EFTB_B_PIN], Pin, (size_t)B * c.Nkin * sizeof(double));
    memcpy(h + e->slot_off[EFTB_B_F], f, (size_t)B * sizeof(double));
    if (c.with_ap) {
        memcpy(h + e->slot_off[EFTB_B_DA], DA, (size_t)B * sizeof(double));
        memcpy(h + e->slot_off[EFTB_B_H], H, (size_t)B * sizeof(double));
    }
    if (bias) memcpy(h + e->slot_off[EFTB_B_BIAS], bias, (size_t)B * NROW * sizeof(double));
    if (rows) {  // packed [B][nG+1][24] -> device rows of MARG_NG1
        const int ng1 = e->like_nG + 1;
        for (int w = 0; w < B; ++w)
            memcpy(h + e->slot_off[EFTB_B_GROWS] + (size_t)w * MARG_NG1 * NROW, rows + (size_t)w * ng1 * NROW, (size_t)ng1 * NROW * sizeof(double));
    }
}

// ... and the device part (issued by the caller's thread or by the submission thread): n queued steps become ONE launch on the next device set --
// their staging blocks are gathered into the set's input block row after row by one upload kernel, then every stage runs on the joint batch.
// plan_launch decides, one function per phase acts; what only the run knows (back_pending, plk_host_written, cur_nl /
// cur_nx) is read behind run_stages, never in the plan.

// how the P_l of a staged launch reaches host memory
enum class PlkExit {
    none,         // it does not: no REDUCE in the mask, or a communicator (P_l stays in device memory for the exchange)
    stored,       // the kernel that forms it also stores it to the set's mapped host block: latency mode (one kernel less on the dependent sampler's
                  // chain) and the node quadrature (round 3 stored from ap_plk_kernel: 1.6 MB of 8-byte PCIe stores kept every SIMD's waves
                  // resident for ~25 us, which is why pipelined steps do not).  A run whose last kernel could not (plk_host_written) leaves by copy_by
    copy_kernel,  // copy16_kernel / copy8_kernel behind the launch (EFTB_PLK_DMA=0)
    dma,          // the DMA engine, in line behind the launch's last kernel (same-box A/B over 200 steps: 0.091-0.096 ms per step against 0.102-0.104
                  // with copy16_kernel -- the what-if runs priced the kernel's PCIe stores at a fifth of the step)
};

struct LaunchPlan {
    int q = 0, lr = 0;              // device set of the launch; slot of its upload events and of lring_set
    unsigned long long L = 0;       // launch number
    int mask = 0, Bt = 0;           // Bt: cosmologies of all steps together
    bool has_rows = false, lat = false;
    // the upload goes where the launch's first kernels go: direct-P_l launches start on the side stream (their front), so the upload in front of
    // them on the same queue needs no cross-queue hand-over (20-35 us each on this runtime, and the chain of a launch has four more)
    hipStream_t up = nullptr;
    PlkExit leave = PlkExit::none;
    PlkExit copy_by = PlkExit::dma;  // dma or copy_kernel: how a copy behind the launch travels
    bool own_dst = false;            // a step names its own destination (eftb_set_step_output): always a copy behind the launch, one transfer per destination
    bool back_joins_copy = false;    // templates-first launches: whoever joins the back half also waits for the copy
    bool compute_word = false, done_word = false;  // the completion words to write (hipStreamWriteValue64; EFTB_DONE_WORDS)
};

static void plan_launch(const eftb_engine* e, const eftb_engine::SubCmd* cmds, int n, bool lat, LaunchPlan* p) {
    p->q = (e->cur_set + 1) % eftb_engine::NSETS;
    p->L = e->launch_seq;
    p->lr = (int)(p->L % eftb_engine::NLRING);
    p->mask = cmds[0].mask;
    p->has_rows = cmds[0].has_rows != 0;
    p->lat = lat;
    for (int j = 0; j < n; ++j) {
        p->Bt += cmds[j].B;
        p->own_dst = p->own_dst || cmds[j].out != nullptr;
    }
    p->up = (e->plk_direct && !lat && e->upload_on_side) ? e->side : e->cpy;
    // latency mode: one queue for the whole step; P_l goes to mapped host memory from the kernel that forms it (REDUCE, or the AP epilogue)
    // unless the NNLO pass adds to it afterwards
    const bool has_plk = e->plk_host[p->q] && (p->mask & EFTB_S_REDUCE);
    const bool direct = has_plk && (lat || (e->plk_direct && !e->comm)) && !e->c.with_nnlo;
    if (direct) {
        p->copy_by = e->plk_dma ? PlkExit::dma : PlkExit::copy_kernel;
        p->leave = (lat || e->ap_plk_nodes) && !p->own_dst ? PlkExit::stored : p->copy_by;
    } else if (has_plk) {
        p->leave = PlkExit::dma;
        p->back_joins_copy = true;
    }
    p->compute_word = e->done_words && !lat;   // compute finished: what the submission thread's flow control counts (the copy-out is not part of it)
    p->done_word = e->done_words;
}

static UploadLayout upload_layout(const eftb_engine* e, bool has_rows) {
    UploadLayout lay{};
    const size_t width[STAGED_ARRAYS] = {(size_t)e->c.Nkin, 1, 1, 1, (size_t)NROW, (size_t)MARG_NG1 * NROW};
    for (int a = 0; a < STAGED_ARRAYS; ++a) {
        const int id = kStagedIn[a];
        lay.width[a] = width[a];
        lay.slot_off[a] = e->slot_off[id];
        lay.stage_off[a] = e->stage_off[id];
        lay.present[a] = e->buf_elems[id] && (id != EFTB_B_GROWS || has_rows);
    }
    return lay;
}

// the staging blocks of the group -> the set's input block, and the events that say so
// (an upload kernel reading the mapped staging blocks, not a DMA transfer: 0.4 MB is latency, and the DMA form measured the same or worse)
// only what was staged travels: P_lin, f, DA, H, the bias rows -- and the likelihood rows (0.6 MB at 128 walkers) when there are any.  Reads
// of host memory from a kernel run at ~16 GB/s: the whole 0.85 MB block took 48-53 us, on the critical path of a dependent sampler
static int launch_upload(eftb_engine* e, const LaunchPlan& p, const eftb_engine::SubCmd* cmds, int n) {
    HIPCHK(hipStreamWaitEvent(p.up, e->evSetDone[p.q], 0));  // the last launch on this set (and the fetch of its results) is over
    const UploadLayout lay = upload_layout(e, p.has_rows);
    int B[MAX_COALESCE];
    for (int j = 0; j < n; ++j) B[j] = cmds[j].B;
    auto gather = [&](int lo, int hi, hipStream_t st) {  // arrays kStagedIn[lo .. hi) of every step of the group
        const UploadSegs us = upload_segments(lay, B, n, lo, hi);
        StageSegs sg{};
        for (; sg.n < us.n; ++sg.n) {
            const UploadSeg& u = us.s[sg.n];
            sg.s[sg.n] = StageSeg{e->stage_host[cmds[u.step].slot] + u.src_off, e->setblock[p.q] + u.dst_off, u.n, u.first};
        }
        if (sg.n && !WHATIF_SKIP(1024)) hipLaunchKernelGGL(stage_gather_kernel, dim3((us.total + 255) / 256), dim3(256), 0, st, sg);
    };
    e->trace_slot = -1;
    if (e->trace_on && !p.lat && e->evTraceBase) {
        e->trace_slot = (int)(e->trace_n++ % eftb_engine::NTRACE);
        e->trace_B[e->trace_slot] = p.Bt;
        e->trace_launch[e->trace_slot] = p.L;
        trace_point(e, 0, p.up);
    }
    e->set_latency[p.q] = p.lat;
    if (p.lat) {
        // the small arrays go first and on the compute queue itself (in line in front of the step's kernels: no cross-queue hand-over; the
        // GPU is idle, nothing of an earlier step can still be reading the set): they are all the step's first kernels wait for -- its first
        // kernel reads P_lin from the staging block itself, whose device copy follows on the copy queue
        gather(1, STAGED_ARRAYS, e->stream);
        HIPCHK(hipEventRecord(e->evStagedR[p.lr], e->stream));
        gather(0, 1, p.up);
        HIPCHK(hipEventRecord(e->evStagedAllR[p.lr], p.up));
    } else {
        gather(0, STAGED_ARRAYS, p.up);
        trace_point(e, 9, p.up);
        HIPCHK(hipEventRecord(e->evStagedR[p.lr], p.up));
    }
    return 0;
}

// the set becomes current: the steps' records, the engine's buffer pointers, the set's flags, and the streams behind the upload
static int bind_set(eftb_engine* e, const LaunchPlan& p, const eftb_engine::SubCmd* cmds, int n) {
    e->cur_set = p.q;
    e->lring_set[p.lr] = p.q;
    ++e->launch_seq;
    int row = 0;
    for (int j = 0; j < n; ++j) {  // where each step's rows will be (the fetch needs it even when the launch fails below: to say so)
        eftb_engine::StepRec& r = e->rec[cmds[j].step % eftb_engine::SUBREC];
        r.set = p.q; r.row = row; r.B = cmds[j].B; r.launch = p.L; r.rc = 0; r.out = cmds[j].out;
        row += cmds[j].B;
    }
    for (int id : kStagedIds)
        if (e->setbuf[p.q][id]) e->buf[id] = e->setbuf[p.q][id];
    e->status[2 * p.q] = e->status[2 * p.q + 1] = 0;  // (whatever an abandoned step left in this set's flags is void)
    ++e->epoch;  // (captured graphs hold the other set's pointers)
    const hipStream_t staged_on = p.lat ? e->stream : p.up;   // (where evStagedR was recorded: that stream is behind it already -- a call saved per launch)
    if (staged_on != e->stream) HIPCHK(hipStreamWaitEvent(e->stream, e->evStagedR[p.lr], 0));  // the side stream forks from here, so it inherits the wait
    if (staged_on != e->pre) HIPCHK(hipStreamWaitEvent(e->pre, e->evStagedR[p.lr], 0));
    if (staged_on != e->side) HIPCHK(hipStreamWaitEvent(e->side, e->evStagedR[p.lr], 0));
    return 0;
}

// what run_stages reads from the engine about the staged launch around it, set here and put back on every way out: this launch's kernels
// raise this set's flags; a latency-mode step reads P_lin from the page-locked staging block (its device copy arrives behind evStagedAllR),
// a pipelined one has settled inputs and may use the back stream; plk_host_out is where a storing kernel puts P_l
struct StagedRunScope {
    eftb_engine* e;
    double* pin_dev;
    StagedRunScope(eftb_engine* e_, const LaunchPlan& p, double* pin_host) : e(e_), pin_dev(e_->buf[EFTB_B_PIN]) {
        e->status_slot = p.q;
        if (p.lat) e->buf[EFTB_B_PIN] = pin_host;
        e->lat_run = p.lat;
        e->plk_host_out = p.leave == PlkExit::stored ? e->plk_host[p.q] : nullptr;
        e->inputs_settled = e->allow_back = !p.lat;
    }
    ~StagedRunScope() {
        e->inputs_settled = e->allow_back = false;
        e->lat_run = false;
        e->plk_host_out = nullptr;
        e->buf[EFTB_B_PIN] = pin_dev;
        e->status_slot = eftb_engine::NSETS;
    }
    StagedRunScope(const StagedRunScope&) = delete;
    StagedRunScope& operator=(const StagedRunScope&) = delete;
};

// P_l [rows of the launch][nl][nx] to host memory on stream st: the set's own page-locked block, or -- per step -- the caller's page-locked array
// (merge_out_spans: which steps share a transfer)
static int copy_out(eftb_engine* e, const LaunchPlan& p, const eftb_engine::SubCmd* cmds, int n, PlkExit by, hipStream_t st) {
    constexpr int copy_wgs = 48;   // (8 ... 512 workgroups measured the same: the kernel's time is the PCIe transfer)
    const size_t per = (size_t)e->cur_nl * e->cur_nx;
    // (16 bytes per lane only where both ends are 16-byte aligned: with an odd row length the later steps of a launch start at odd offsets)
    auto launch_copy = [&](const double* src, double* dst, size_t count) {
        if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0)
            hipLaunchKernelGGL(copy16_kernel, dim3(copy_wgs), dim3(256), 0, st, src, dst, count);
        else hipLaunchKernelGGL(copy8_kernel, dim3(copy_wgs), dim3(256), 0, st, src, dst, count);
    };
    if (WHATIF_SKIP(512)) return 0;   // (what-if: P_l stays on the device)
    if (WHATIF_SKIP(2048) && e->PLK0) {   // (what-if: the copy kernel with a device destination -- the stream holds it, PCIe does not)
        launch_copy(e->buf[EFTB_B_PLK], e->PLK0, (size_t)p.Bt * per);
        return 0;
    }
    const double* out[MAX_COALESCE];
    int B[MAX_COALESCE];
    for (int j = 0; j < n; ++j) {
        if (cmds[j].out && cmds[j].out_count < (size_t)cmds[j].B * per)
            return fail("eftb_run_staged: the step's P_l has %zu elements, the destination of eftb_set_step_output holds %zu", (size_t)cmds[j].B * per, cmds[j].out_count);
        out[j] = cmds[j].out;
        B[j] = cmds[j].B;
    }
    OutSpan spans[MAX_COALESCE];
    const int ns = merge_out_spans(out, B, n, per, spans);
    for (int i = 0; i < ns; ++i) {
        const OutSpan& s = spans[i];
        const double* src = e->buf[EFTB_B_PLK] + (size_t)s.row * per;
        double* dst = s.own ? cmds[s.step].out : e->plk_host[p.q] + (size_t)s.row * per;
        if (by == PlkExit::dma) HIPCHK(hipMemcpyAsync(dst, src, (size_t)s.rows * per * sizeof(double), hipMemcpyDeviceToHost, st));
        else launch_copy(src, dst, (size_t)s.rows * per);
    }
    return 0;
}

// compute finished: written behind the launch's last kernel, in front of the copy-out
static void signal_compute_done(eftb_engine* e, const LaunchPlan& p, hipStream_t last) {
    if (!p.compute_word) return;
    if (hipStreamWriteValue64(last, const_cast<unsigned long long*>(e->set_done) + eftb_engine::NSETS + p.q, p.L + 1, 0) == hipSuccess) e->set_cword[p.q] = p.L + 1;
    else (void)hipGetLastError();
}

// everything finished: the set's event and, behind it, the set's completion word
static int signal_done(eftb_engine* e, const LaunchPlan& p, hipStream_t last) {
    trace_point(e, 8, last);
    e->trace_slot = -1;
    HIPCHK(hipEventRecord(e->evSetDone[p.q], last));
    if (e->back_pending && p.back_joins_copy) HIPCHK(hipEventRecord(e->evBack[(e->back_step + 1) & 1], last));
    if (p.done_word) {
        if (hipStreamWriteValue64(last, const_cast<unsigned long long*>(e->set_done) + p.q, p.L + 1, 0) == hipSuccess) e->set_word[p.q] = p.L + 1;
        else {
            (void)hipGetLastError();
            e->done_words = false;  // this runtime refuses the command: event queries from here on (the words of the earlier launches stay valid)
        }
    }
    return 0;
}

static int issue_group(eftb_engine* e, const eftb_engine::SubCmd* cmds, int n, bool lat) {
    LaunchPlan p;
    plan_launch(e, cmds, n, lat, &p);
    if (int rc = launch_upload(e, p, cmds, n)) return rc;
    if (int rc = bind_set(e, p, cmds, n)) return rc;
    {
        StagedRunScope scope(e, p, e->stage_host[cmds[0].slot] + e->slot_off[EFTB_B_PIN]);
        if (int rc = run_stages(e, p.mask, p.Bt)) { e->trace_slot = -1; return rc; }
    }
    for (int j = 0; j < n; ++j) {  // shape of the output rows (after the pipeline operator, if the mask has one)
        eftb_engine::StepRec& r = e->rec[cmds[j].step % eftb_engine::SUBREC];
        r.nl = e->cur_nl; r.nx = e->cur_nx;
    }
    const hipStream_t last = e->back_pending ? e->back : e->stream;  // the launch ends where its back half ran: the copy-out, the set's event and its word follow there
    if (lat) HIPCHK(hipStreamWaitEvent(last, e->evStagedAllR[p.lr], 0));  // (the set is not "done" before its own upload is)
    signal_compute_done(e, p, last);
    const PlkExit by = p.leave == PlkExit::stored ? (e->plk_host_written ? PlkExit::none : p.copy_by) : p.leave;
    if (by != PlkExit::none)
        if (int rc = copy_out(e, p, cmds, n, by, last)) return rc;
    return signal_done(e, p, last);
}

// issue_group + bookkeeping shared by both issuing threads: the steps' records, the clocks, the publication of "issued"
static int issue_and_publish(eftb_engine* e, const eftb_engine::SubCmd* cmds, int n, bool lat, bool by_caller) {
    const auto ti0 = std::chrono::steady_clock::now();
    const int q_before = e->cur_set;
    const unsigned long long L_before = e->launch_seq;
    const int rc = issue_group(e, cmds, n, lat);
    if (rc && e->launch_seq == L_before) {  // failed before the set was taken: the steps still need records that say so
        for (int j = 0; j < n; ++j) {
            eftb_engine::StepRec& r = e->rec[cmds[j].step % eftb_engine::SUBREC];
            r.set = q_before; r.row = 0; r.B = cmds[j].B; r.launch = ~0ull; r.out = cmds[j].out;
        }
    }
    for (int j = 0; j < n; ++j) {
        const int ri = (int)(cmds[j].step % eftb_engine::SUBREC);
        e->rec[ri].rc = rc;
        if (rc) snprintf(e->sub_err[ri], sizeof e->sub_err[ri], "%s", g_err.c_str());
    }
    if (e->sub_stats) {
        e->issue_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - ti0).count();
        e->issue_n += n;
        ++e->launch_n;
        if (by_caller) e->inline_n += n;
    }
    e->steps_launched.store(cmds[n - 1].step + 1, std::memory_order_release);
    return rc;
}

// The one completion rule.  What says that launch L on set q has finished: its compute-done word if one was enqueued and the compute is all that
// is asked about (the copy-out of P_l may still run), else its done word if one was enqueued, else the set's event (EFTB_DONE_WORDS=0, or the
// runtime refused the write).  Words grow with the launch number: a later launch on the set says it too.
// done_word_of: the word in mapped memory that says so once it has reached L + 1, or null: ask the event.  (A caller that spins takes the pointer
// once and polls that word alone -- set_word / set_cword share cache lines with what the issuing thread writes at every launch.)
static inline const volatile unsigned long long* done_word_of(const eftb_engine* e, int q, unsigned long long L, bool compute_only) {
    if (compute_only && e->set_cword[q] >= L + 1) return e->set_done + eftb_engine::NSETS + q;
    return e->set_word[q] >= L + 1 ? e->set_done + q : nullptr;
}
static bool launch_over(eftb_engine* e, int q, unsigned long long L, bool compute_only) {
    const volatile unsigned long long* w = done_word_of(e, q, L, compute_only);
    return w ? *w >= L + 1 : hipEventQuery(e->evSetDone[q]) == hipSuccess;
}

// has the compute of staged launch L finished?  (issuing thread: what its flow control counts)
static bool launch_finished(eftb_engine* e, unsigned long long L) { return launch_over(e, e->lring_set[L % eftb_engine::NLRING], L, true); }

// ---- submission thread (see eftb_engine::SubCmd)
static void sub_main(eftb_engine* e) {
    (void)hipSetDevice(e->c.device);
    unsigned long long head = e->sub_head.load(std::memory_order_relaxed);
    for (;;) {
        // wait for a command: spin for a while (a pipelined loop delivers one every ~0.1 ms), then sleep
        unsigned spins = 0;
        while (e->sub_tail.load(std::memory_order_acquire) == head) {
            if (e->sub_stop.load(std::memory_order_acquire)) return;
            if (++spins < 200000) { cpu_pause(); continue; }   // ~ a few ms
            std::unique_lock<std::mutex> lk(e->sub_mx);
            e->sub_sleeping.store(true, std::memory_order_seq_cst);
            e->sub_cv.wait(lk, [&] { return e->sub_tail.load(std::memory_order_acquire) != head || e->sub_stop.load(std::memory_order_acquire); });
            e->sub_sleeping.store(false, std::memory_order_seq_cst);
            spins = 0;
        }
        while (e->sub_hold.load(std::memory_order_acquire) && !e->sub_stop.load(std::memory_order_acquire)) cpu_pause();
        // flow control: with sub_inflight launches still running the queue is left to grow -- what has piled up by the time one of them finishes
        // leaves as one launch (coalesce_max steps at most)
        while (e->launch_done < e->launch_seq && launch_finished(e, e->launch_done)) ++e->launch_done;
        auto go = [&] {
            for (;; ++e->launch_done) {
                const long long inflight = (long long)(e->launch_seq - e->launch_done);
                // go: below the in-flight limit AND (a full group is waiting, or the GPU is about to run dry: fewer than sub_low launches left)
                if (inflight < e->sub_inflight &&
                    (inflight < e->sub_low || (long long)(e->sub_tail.load(std::memory_order_acquire) - head) >= e->coalesce_max ||
                     e->sub_flush.load(std::memory_order_acquire))) return true;
                if (inflight <= 0 || !launch_finished(e, e->launch_done)) return false;
            }
        };
        // (a launch that never finishes must not hold the queue -- and with it every entry point that drains it -- for ever: on a time-out the
        // steps go out anyway and their fetches report it)
        (void)spin_until([&] { return go() || e->sub_stop.load(std::memory_order_acquire); }, 0xffff, 16);
        eftb_engine::SubCmd grp[MAX_COALESCE];
        int n = 0, Bt = 0;
        const unsigned long long tail = e->sub_tail.load(std::memory_order_acquire);
        while (head + n < tail && n < e->coalesce_max) {
            const eftb_engine::SubCmd& c = e->sub_ring[(head + n) % eftb_engine::SUBQ];
            if (n && (c.mask != grp[0].mask || c.has_rows != grp[0].has_rows || Bt + c.B > e->c.max_batch || e->check_finite)) break;
            grp[n++] = c;
            Bt += c.B;
        }
        (void)issue_and_publish(e, grp, n, false, false);
        head += n;
        if (head == e->sub_tail.load(std::memory_order_acquire)) e->sub_flush.store(false, std::memory_order_release);  // (a step queued from here on waits for its group again)
        e->sub_head.store(head, std::memory_order_release);
    }
}

// nothing queued and the submission thread between commands: the engine's state belongs to the caller's thread
static inline bool sub_quiescent(const eftb_engine* e) {
    return e->sub_head.load(std::memory_order_acquire) == e->sub_tail.load(std::memory_order_relaxed);
}

static inline void sub_drain(eftb_engine* e) {
    if (!e->sub_started) return;
    e->sub_hold.store(false, std::memory_order_release);   // (an entry point that needs the queue empty ends a test's hold)
    while (!sub_quiescent(e)) cpu_pause();
}

static void sub_stop_thread(eftb_engine* e) {
    if (!e->sub_started) return;
    sub_drain(e);
    {
        std::lock_guard<std::mutex> lk(e->sub_mx);
        e->sub_stop.store(true, std::memory_order_release);
    }
    e->sub_cv.notify_all();
    if (e->sub_thread.joinable()) e->sub_thread.join();
    e->sub_started = false;
}

// waits until the launch of staged step `step` has been issued, and reports its launch error (if any) as this call's
static int sub_wait_launched(eftb_engine* e, unsigned long long step, const char* who) {
    auto issued = [&] { return e->steps_launched.load(std::memory_order_acquire) > step; };
    if (!issued() && !spin_until(issued, 0xffff))   // (the usual case takes no clock reading)
        return fail("%s: the submission thread did not issue the step within %.0f s (EFTB_FETCH_TIMEOUT_S)", who, fetch_timeout_s());
    const int r = (int)(step % eftb_engine::SUBREC);
    if (e->rec[r].rc) return fail("%s: the launch of this step failed: %s", who, e->sub_err[r]);
    return 0;
}

int eftb_stage_inputs(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA, const double* H, const double* bias,
                      const double* rows) {
    if (!e || !Pin || !f) {
        if (e) e->stg_out = nullptr;
        return fail("eftb_stage_inputs: null argument");
    }
    struct OutGuard {   // a step that is refused here takes the destination named for it (eftb_set_step_output) with it: it must not pass to the next step
        eftb_engine* e;
        bool staged = false;
        ~OutGuard() { if (!staged) e->stg_out = nullptr; }
    } guard{e};
    if (!e->finalized) return fail("eftb_stage_inputs: engine not finalized");
    const eftb_config& c = e->c;
    const int step_max = c.step_batch > 0 ? c.step_batch : c.max_batch;
    if (B < 1 || B > step_max) return fail("eftb_stage_inputs: batch %d outside [1, %d]", B, step_max);
    if (c.with_ap && (!DA || !H)) return fail("eftb_stage_inputs: DA and H are required when with_ap=1");
    if (rows && !e->like_ndata) return fail("eftb_stage_inputs: rows need eftb_set_likelihood");
    if (int rc = validate_inputs(c, "eftb_stage_inputs", B, Pin, f, DA, H)) return rc;
    if (!e->cpy) {
        sub_drain(e);
        if (int rc = staged_setup(e)) return rc;
    }
    HIPCHK(hipSetDevice(c.device));
    const int slot = (int)(e->steps_submitted % eftb_engine::NSLOT);  // the oldest staging block: its step was fetched (or abandoned) long ago
    // the step that used this block last has been issued (its events exist) ...
    if (e->slot_step[slot]) {
        (void)sub_wait_launched(e, e->slot_step[slot] - 1, "eftb_stage_inputs");  // (a failed launch left nothing to wait for; its fetch reports it)
        const eftb_engine::StepRec& r = e->rec[(e->slot_step[slot] - 1) % eftb_engine::SUBREC];
        // (a launch whose completion word has been written is over, its upload with it: no runtime call -- hipEventSynchronize costs this thread 6 us per step)
        if (r.launch != ~0ull && !launch_over(e, r.set, r.launch, false)) {
            const int lr = (int)(r.launch % eftb_engine::NLRING);
            // ... and the block is free again (the upload from it has finished; a latency-mode step's first kernel read P_lin from the block itself:
            // that step must be over too -- it almost always is)
            HIPCHK(hipEventSynchronize(e->slot_latency[slot] ? e->evStagedAllR[lr] : e->evStagedR[lr]));
            if (e->slot_latency[slot])
                if (int rc = spin_event(e->evSetDone[r.set], "eftb_stage_inputs", "the latency-mode step that read this staging block")) return rc;
        }
    }
    // Who issues the step?  With earlier steps still queued or in flight, the submission thread (this call only fills the staging block).  With
    // the engine quiescent and the GPU idle -- a sampler whose next step depends on this step's result -- this thread, at once, as a latency-mode
    // step if that is enabled (see latency_auto)
    const bool quiet = sub_quiescent(e);
    const bool gpu_idle = quiet && hipEventQuery(e->evSetDone[e->cur_set]) == hipSuccess;
    // (with latency mode off the caller has said that more steps follow at once: queued from the first step on -- the caller goes on staging
    // while the thread issues; 2-3 % of a 20-step loop)
    e->stg_inline = !(e->sub_mode == 2 || (e->sub_mode == 1 && (!gpu_idle || !e->latency_auto)));
    // nothing in flight (the step launched last has finished, or none was launched): the step staged here has the GPU to itself -- see latency_auto
    e->stg_lat = e->stg_inline && e->latency_auto && gpu_idle && e->slot_off[EFTB_B_PIN] == 0;
    e->slot_latency[slot] = e->stg_lat;
    if (e->stg_lat) {
        sub_drain(e);
        hipLaunchKernelGGL(wake_kernel, dim3(1), dim3(64), 0, e->stream);  // (see wake_kernel: its start-up runs under the host copies below)
    }
    const auto tf0 = std::chrono::steady_clock::now();
    stage_fill(e, slot, B, Pin, f, DA, H, bias, rows);
    if (e->sub_stats) e->fill_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - tf0).count();
    e->stg_slot = slot; e->stg_B = B; e->stg_rows = rows ? 1 : 0;
    guard.staged = true;
    return 0;
}

int eftb_flush(eftb_engine* e) {
    if (!e) return fail("eftb_flush: null engine");
    if (e->sub_started && !sub_quiescent(e)) e->sub_flush.store(true, std::memory_order_release);
    return 0;
}

int eftb_set_step_output(eftb_engine* e, double* dst, size_t count) {
    if (!e) return fail("eftb_set_step_output: null engine");
    if (!dst) { e->stg_out = nullptr; e->stg_out_count = 0; return 0; }
    if (e->comm) return fail("eftb_set_step_output: P_l of an engine with a communicator stays in device memory for the exchange (eftb_gathered_view)");
    HIPCHK(hipSetDevice(e->c.device));
    // the DMA engine writes the array behind the step: it must be page-locked (eftb_host_alloc or the runtime's own page-locked allocation or registration) -- pageable memory would
    // turn every transfer into a synchronous staged copy on the issuing thread
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, dst) != hipSuccess || at.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return fail("eftb_set_step_output: the destination is not page-locked host memory (allocate it with eftb_host_alloc / Engine.pinned_empty)");
    }
    e->stg_out = dst;
    e->stg_out_count = count;
    return 0;
}

int eftb_run_staged(eftb_engine* e, int mask, int B) {
    if (!e) return fail("eftb_run_staged: null engine");
    if (!e->cpy || e->stg_slot < 0) return fail("eftb_run_staged: nothing staged (eftb_stage_inputs first)");
    if (B != e->stg_B) return fail("eftb_run_staged: batch %d, but %d cosmologies were staged", B, e->stg_B);
    HIPCHK(hipSetDevice(e->c.device));
    e->templ_ok = false;  // (a staged step rotates the template blocks: eftb_draws_* refuse until the next template-producing run / eftb_put)
    ++e->draw_gen;
    const unsigned long long step = e->steps_submitted;
    double* out = e->stg_out;
    e->stg_out = nullptr;   // (one step only, launched or not)
    if (out) {
        if (!(mask & EFTB_S_REDUCE) || (mask & EFTB_S_LOGP)) return fail("eftb_run_staged: eftb_set_step_output names a destination for P_l, but this run forms none (mask 0x%x)", mask);
        if (!e->plk_host[0]) return fail("eftb_run_staged: eftb_set_step_output needs an engine whose P_l leaves through the copy-out (no communicator)");
    }
    const eftb_engine::SubCmd cmd{e->stg_slot, mask, B, e->stg_rows, step, out, e->stg_out_count};
    int rc = 0;
    if (!e->stg_inline) {  // queued: the submission thread uploads the staging block and launches the step (with whatever else is queued by then)
        if (!e->sub_started) {
            e->sub_stop.store(false);
            e->sub_thread = std::thread(sub_main, e);
            e->sub_started = true;
        }
        // (never more than NSLOT - 1 pending: each owns a staging block, and eftb_stage_inputs has waited for the block's previous user)
        const unsigned long long tail = e->sub_tail.load(std::memory_order_relaxed);
        e->sub_ring[tail % eftb_engine::SUBQ] = cmd;
        e->sub_tail.store(tail + 1, std::memory_order_release);
        if (e->sub_sleeping.load(std::memory_order_seq_cst)) {
            std::lock_guard<std::mutex> lk(e->sub_mx);
            e->sub_cv.notify_one();
        }
    } else {
        sub_drain(e);
        // (launch bookkeeping of the issuing thread: bring "finished" up to date, as the submission thread does before its launches)
        while (e->launch_done < e->launch_seq && launch_finished(e, e->launch_done)) ++e->launch_done;
        rc = issue_and_publish(e, &cmd, 1, e->stg_lat, true);
    }
    e->slot_step[e->stg_slot] = step + 1;
    e->stg_slot = -1;
    ++e->steps_submitted;
    return rc;
}

// the launch that carried a step has finished (its completion word, or its set's event)
static int wait_step_done(eftb_engine* e, const eftb_engine::StepRec& r, const char* who) {
    const auto tw0 = std::chrono::steady_clock::now();
    int rc = 0;
    const int t = r.set;
    if (const volatile unsigned long long* w = done_word_of(e, t, r.launch, false)) {   // (else: no completion write was enqueued for this launch)
        const unsigned long long want = r.launch + 1;
        if (!spin_until([w, want] { return *w >= want; }, 0xfffff, 1, tw0))
            rc = fail("%s: the step did not finish within %.0f s (EFTB_FETCH_TIMEOUT_S)", who, fetch_timeout_s());
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        rc = spin_event(e->evSetDone[t], who, "the step");
    }
    if (e->sub_stats) e->wait_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - tw0).count();
    return rc;
}

// record of the staged step `back` steps before the one submitted last, once its launch has been issued
static int staged_step(eftb_engine* e, const char* who, int back, const eftb_engine::StepRec** rec) {
    if (back < 0 || back >= eftb_engine::NSETS) return fail("%s: back must be 0 (the step launched last) ... %d (that many steps before it)", who, eftb_engine::NSETS - 1);
    if (!e->cpy) return fail("%s: no staged run yet", who);
    if ((unsigned long long)back >= e->steps_submitted)
        return fail("%s: back = %d, but only %llu staged step(s) have been launched", who, back, e->steps_submitted);
    const unsigned long long step = e->steps_submitted - 1 - back;
    if (int rc = sub_wait_launched(e, step, who)) return rc;
    *rec = &e->rec[step % eftb_engine::SUBREC];
    return 0;
}

// where a step's rows of a per-set output block start: P_l [row][nl][nx]; ln P per likelihood point [row / ntr][MARG_OUT]
static inline size_t step_offset(const eftb_engine* e, const eftb_engine::StepRec& r, int id) {
    return id == EFTB_B_PLK ? (size_t)r.row * r.nl * r.nx : (size_t)(r.row / e->ntr) * MARG_OUT;
}

// front half of both fetches: the step's record once its launch has finished, and where its rows start in the set's block.  count: elements the
// caller wants copied (a view: 0); view: the block itself is handed out, so it has to be in host memory
static int fetch_front(eftb_engine* e, const char* who, int back, int id, size_t count, bool view, const eftb_engine::StepRec** rec, size_t* off) {
    if (id != EFTB_B_PLK && id != EFTB_B_LOGP) return fail("%s: only EFTB_B_PLK and EFTB_B_LOGP are per-set outputs", who);
    if (count > e->buf_elems[id]) return fail("%s: buffer %d holds %zu elements, asked %zu", who, id, e->buf_elems[id], count);
    if (int rc = staged_step(e, who, back, rec)) return rc;
    HIPCHK(hipSetDevice(e->c.device));
    if (view && id == EFTB_B_PLK && !e->plk_host[(*rec)->set])
        return fail("%s: P_l of this engine stays in device memory for the RCCL exchange (eftb_gathered_view hands out the gathered block)", who);
    if (int rc = wait_step_done(e, **rec, who)) return rc;
    *off = step_offset(e, **rec, id);
    return 0;
}

// the step's P_l went to the caller's own array (eftb_set_step_output), this many doubles of it
static inline bool step_own_plk(const eftb_engine::StepRec& r, int id, size_t* elems) {
    *elems = (size_t)r.B * r.nl * r.nx;
    return id == EFTB_B_PLK && r.out;
}

int eftb_fetch_back(eftb_engine* e, int back, int id, double* host, size_t count) {
    if (!e || !host) return fail("eftb_fetch_back: null argument");
    const eftb_engine::StepRec* r = nullptr;
    size_t off = 0, own = 0;
    if (int rc = fetch_front(e, "eftb_fetch_back", back, id, count, false, &r, &off)) return rc;
    const int t = r->set;
    if (off + count > e->buf_elems[id]) return fail("eftb_fetch_back: the step's rows start at element %zu of %zu, asked %zu", off, e->buf_elems[id], count);
    if (step_own_plk(*r, id, &own)) {
        if (count > own) return fail("eftb_fetch_back: the step's P_l has %zu elements, asked %zu", own, count);
        if (host != r->out) memcpy(host, r->out, count * sizeof(double));
    } else if (id == EFTB_B_PLK && e->plk_host[t])
        memcpy(host, e->plk_host[t] + off, count * sizeof(double));  // copied out behind the step
    else if (id == EFTB_B_PLK)  // multi-GPU runs keep P_l on the device for the RCCL exchange
        HIPCHK(hipMemcpy(host, e->setbuf[t][id] + off, count * sizeof(double), hipMemcpyDeviceToHost));
    else
        memcpy(host, e->setbuf[t][id] + off, count * sizeof(double));  // ln P is already in (mapped) host memory
    return check_status(e, "eftb_fetch_back", t);  // this launch's own flags only: the steps queued behind it report with their own fetch
}

int eftb_fetch_previous(eftb_engine* e, int id, double* host, size_t count) { return eftb_fetch_back(e, 1, id, host, count); }

int eftb_fetch_view(eftb_engine* e, int back, int id, const double** block, size_t* count) {
    if (!e || !block) return fail("eftb_fetch_view: null argument");
    const eftb_engine::StepRec* r = nullptr;
    size_t off = 0, own = 0;
    if (int rc = fetch_front(e, "eftb_fetch_view", back, id, 0, true, &r, &off)) return rc;
    const int t = r->set;
    const bool own_plk = step_own_plk(*r, id, &own);   // (then the caller's array is the block)
    *block = own_plk ? r->out : (id == EFTB_B_PLK ? e->plk_host[t] : e->setbuf[t][id]) + off;
    if (count) *count = own_plk ? own : e->buf_elems[id] - off;
    return check_status(e, "eftb_fetch_view", t);
}

int eftb_submit_stats(eftb_engine* e, int enable, int reset, double out[6]) {
    if (!e) return fail("eftb_submit_stats: null engine");
    sub_drain(e);
    if (out) {
        out[0] = (double)e->issue_n; out[1] = (double)e->inline_n; out[2] = e->issue_ns * 1e-3; out[3] = e->fill_ns * 1e-3; out[4] = e->wait_ns * 1e-3;
        out[5] = (double)e->launch_n;
    }
    if (reset) { e->issue_n = e->inline_n = e->launch_n = 0; e->issue_ns = e->fill_ns = e->wait_ns = 0.0; }
    e->sub_stats = enable != 0;
    return 0;
}

int eftb_step_trace(eftb_engine* e, double* out, int max_launches, int* n_out) {
    if (!e || !out || !n_out) return fail("eftb_step_trace: null argument");
    sub_drain(e);
    HIPCHK(hipSetDevice(e->c.device));
    if (!e->evTraceBase) return fail("eftb_step_trace: EFTB_O_STEP_TRACE was never switched on");
    HIPCHK(sync_all(e));
    const unsigned long long total = e->trace_n, first = total > (unsigned long long)eftb_engine::NTRACE ? total - eftb_engine::NTRACE : 0;
    int n = 0;
    for (unsigned long long i = first; i < total && n < max_launches; ++i) {
        const int sl = (int)(i % eftb_engine::NTRACE);
        double* row = out + (size_t)n * (eftb_engine::NTP + 2);
        row[0] = (double)e->trace_launch[sl];
        row[1] = (double)e->trace_B[sl];
        bool ok = true;
        for (int p = 0; p < eftb_engine::NTP; ++p) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e->evTraceBase, e->evTrace[sl][p]) != hipSuccess) { (void)hipGetLastError(); ok = false; ms = -1.f; }
            row[2 + p] = ms * 1e3;
        }
        (void)ok;
        ++n;
    }
    *n_out = n;
    return 0;
}

int eftb_step(eftb_engine* e, int mask, int B, const double* Pin, const double* f, const double* DA, const double* H, const double* bias,
              const double* rows, int back, int id, const double** block, size_t* count) {
    if (int rc = eftb_stage_inputs(e, B, Pin, f, DA, H, bias, rows)) return rc;
    if (int rc = eftb_run_staged(e, mask, B)) return rc;
    if (block) *block = nullptr;
    if (back < 0 || !block || (unsigned long long)back >= e->steps_submitted) return 0;  // (the pipeline is still filling: nothing to hand out yet)
    return eftb_fetch_view(e, back, id, block, count);
}

int eftb_comm_unique_id(char id[128]) {
    if (!id) return fail("eftb_comm_unique_id: null argument");
    if (int rc = rccl_load()) return rc;
    ncclUniqueId u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    static_assert(sizeof(u) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id, &u, 128);
    return 0;
}

int eftb_comm_init(eftb_engine* e, int nranks, int rank, const char id[128]) {
    if (e) sub_drain(e);
    if (!e || !id) return fail("eftb_comm_init: null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("eftb_comm_init: bad rank %d of %d", rank, nranks);
    if (e->cpy) return fail("eftb_comm_init: call it before the first eftb_stage_inputs (the staged sets place P_l where the exchange can read it)");
    if (int rc = rccl_load()) return rc;
    HIPCHK(hipSetDevice(e->c.device));
    ncclUniqueId u;
    memcpy(&u, id, 128);
    NCCLCHK(g_rccl.CommInitRank(&e->comm, nranks, u, rank));
    e->nranks = nranks;
    e->rank = rank;
    return 0;
}

int eftb_gather_plk(eftb_engine* e, int B, int root, double* host_out) {
    if (e) sub_drain(e);
    if (!e) return fail("eftb_gather_plk: null engine");
    if (B < 1 || B > e->c.max_batch) return fail("eftb_gather_plk: batch %d outside [1, %d]", B, e->c.max_batch);
    if (root < 0 || root >= e->nranks) return fail("eftb_gather_plk: bad root %d", root);
    HIPCHK(hipSetDevice(e->c.device));
    const size_t count = (size_t)B * e->cur_nl * e->cur_nx;
    if (e->rank == root) {
        e->gather_slot = (e->gather_slot + 1) % eftb_engine::NSETS;
        const int q = e->gather_slot;
        if (!e->gathered2[q]) {
            const size_t bytes = (size_t)e->nranks * e->c.max_batch * e->c.Nl * e->c.Nk * sizeof(double);
            HIPCHK(own_dev(e->own, &e->gathered2[q], bytes));
            HIPCHK(own_event(e->own, &e->evGath2[q], hipEventDisableTiming));
            HIPCHK(own_host(e->own, &e->gath_host[q], bytes, hipHostMallocDefault));
            HIPCHK(own_event(e->own, &e->evGathHost[q], hipEventDisableTiming));
        }
        e->gathered = e->gathered2[q];
    }
    // The exchange runs in line on the stream that writes P_l, straight from the P_l buffer: measured 0.018 ms per step, against 0.24 ms on a
    // communication stream of its own behind a snapshot -- the RCCL kernel holds up new dispatches on every queue while it runs, so keeping the
    // compute stream "free" beside it buys nothing, and the look-ahead stream carries the next step's front half anyway.
    const bool on_back = e->back_pending;  // P_l is being written on the back-half stream: the exchange follows it there
    hipStream_t cs = on_back ? e->back : e->stream;
    const double* sendbuf = e->buf[EFTB_B_PLK];
    if (e->nranks == 1 && !e->comm) {
        HIPCHK(hipMemcpyAsync(e->gathered, sendbuf, count * sizeof(double), hipMemcpyDeviceToDevice, cs));
    } else {  // with a communicator even a single rank goes through the RCCL send / recv group (self exchange)
        if (!e->comm) return fail("eftb_gather_plk: eftb_comm_init was not called");
        NCCLCHK(g_rccl.GroupStart());
        if (e->rank == root)
            for (int r = 0; r < e->nranks; ++r) NCCLCHK(g_rccl.Recv(e->gathered + (size_t)r * count, count, ncclDouble, r, e->comm, cs));
        NCCLCHK(g_rccl.Send(sendbuf, count, ncclDouble, root, e->comm, cs));
        NCCLCHK(g_rccl.GroupEnd());
    }
    if (e->rank == root) {
        const int q = e->gather_slot;
        HIPCHK(hipEventRecord(e->evGath2[q], cs));
        e->gath_elems[q] = (size_t)e->nranks * count;
        e->gath_set[q] = e->buf[EFTB_B_PLK] == e->orig[EFTB_B_PLK] || !e->cpy ? eftb_engine::NSETS : e->cur_set;
        // copy-out with the DMA engine, in line behind the exchange (measured with the PCIe traffic of eight ranks, 12.6 MB per step: 0.441 ms
        // per step; on a stream of its own 0.52 ms -- a sixth stream shares a hardware queue with the look-ahead --; a copy kernel writing
        // mapped host memory 0.62 ms)
        HIPCHK(hipMemcpyAsync(e->gath_host[q], e->gathered2[q], e->gath_elems[q] * sizeof(double), hipMemcpyDeviceToHost, cs));
        HIPCHK(hipEventRecord(e->evGathHost[q], cs));
    }
    if (on_back) HIPCHK(hipEventRecord(e->evBack[(e->back_step + 1) & 1], cs));  // whoever joins the back half also waits for the exchange
    if (host_out && e->rank == root) {
        HIPCHK(hipEventSynchronize(e->evGathHost[e->gather_slot]));
        memcpy(host_out, e->gath_host[e->gather_slot], (size_t)e->nranks * count * sizeof(double));
    }
    return 0;
}

// waits for the copy-out of the exchange `which` exchanges back and returns where its block sits in host memory
static int gathered_ready(eftb_engine* e, const char* who, int which, int* slot) {
    if (which < 0 || which >= eftb_engine::NSETS) return fail("%s: `back` must be 0 (the last exchange enqueued) ... %d (that many exchanges before it)", who, eftb_engine::NSETS - 1);
    const int q = (e->gather_slot + eftb_engine::NSETS - which) % eftb_engine::NSETS;
    if (!e->gathered2[q] || !e->gath_elems[q]) return fail("%s: no such exchange yet", who);
    HIPCHK(hipSetDevice(e->c.device));
    if (int rc = spin_event(e->evGathHost[q], who, "the exchange")) return rc;
    *slot = q;
    return check_status(e, who, e->gath_set[q]);  // the flags of the step whose P_l this block carries (the root's own share)
}

int eftb_gathered_view(eftb_engine* e, int which, const double** block, size_t* count) {
    if (!e || !block) return fail("eftb_gathered_view: null argument");
    int q = 0;
    if (int rc = gathered_ready(e, "eftb_gathered_view", which, &q)) return rc;
    *block = e->gath_host[q];
    if (count) *count = e->gath_elems[q];
    return 0;
}

int eftb_fetch_gathered(eftb_engine* e, int which /* = back */, double* host, size_t count) {
    if (!e || !host) return fail("eftb_fetch_gathered: null argument");
    int q = 0;
    if (int rc = gathered_ready(e, "eftb_fetch_gathered", which, &q)) return rc;
    if (count > e->gath_elems[q]) return fail("eftb_fetch_gathered: the exchange holds %zu elements, asked %zu", e->gath_elems[q], count);
    memcpy(host, e->gath_host[q], count * sizeof(double));
    return 0;
}

int eftb_mfma_f64_peak(int device, double* tflops) {
    if (!tflops) return fail("eftb_mfma_f64_peak: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("eftb_mfma_f64_peak: no HIP device visible");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    Ledger own;  // (released when the probe returns, however it returns)
    double* sink = nullptr;
    HIPCHK(own_dev(own, &sink, sizeof(double)));
    hipEvent_t a, b;
    HIPCHK(own_event(own, &a));
    HIPCHK(own_event(own, &b));
    const int iters = 40000, blocks = prop.multiProcessorCount;  // 8 waves per CU = 2 waves per SIMD
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(512), 0, 0, 100, sink);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(a, 0));
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(512), 0, 0, iters, sink);
    HIPCHK(hipEventRecord(b, 0));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double flops = (double)blocks * 8 * iters * 4 * (2.0 * 16 * 16 * 4);
    *tflops = flops / (ms * 1e-3) / 1e12;
    return 0;
}

int eftb_stream_read_probe(int device, size_t bytes, int bytes_per_lane, double* gbps) {
    if (bytes_per_lane != 8 && bytes_per_lane != 16) return fail("eftb_stream_read_probe: bytes_per_lane must be 8 or 16");
    if (bytes < 4096 || bytes > ((size_t)64 << 30)) return fail("eftb_stream_read_probe: bytes out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("eftb_stream_read_probe: no HIP device visible");
    HIPCHK(hipSetDevice(device));
    const size_t n = bytes / sizeof(double) / 2 * 2;
    Ledger own;
    double *src = nullptr, *sink = nullptr;
    HIPCHK(own_dev(own, &src, n * sizeof(double)));
    HIPCHK(own_dev(own, &sink, sizeof(double)));
    HIPCHK(hipMemset(src, 0, n * sizeof(double)));
    hipEvent_t a, b;
    HIPCHK(own_event(own, &a));
    HIPCHK(own_event(own, &b));
    float ms = 0.f;
    for (int rep = 0; rep < 2; ++rep) {  // the second launch is the timed one
        HIPCHK(hipEventRecord(a, 0));
        if (bytes_per_lane == 8) hipLaunchKernelGGL(stream_read_kernel<1>, dim3(4096), dim3(256), 0, 0, src, n, sink);
        else hipLaunchKernelGGL(stream_read_kernel<2>, dim3(4096), dim3(256), 0, 0, src, n, sink);
        HIPCHK(hipEventRecord(b, 0));
        HIPCHK(hipEventSynchronize(b));
        HIPCHK(hipEventElapsedTime(&ms, a, b));
    }
    if (gbps) *gbps = (double)n * sizeof(double) / (ms * 1e-3) / 1e9;
    return 0;
}

/* Window precompute on the device (reference window.py:262-359); see window_bessel_kernel. */
int eftb_window_precompute(int device, int Na, int Nl, int Nk, int nx, int Np, const double* k, const double* x, const double* Qt,
                           const double* T, const double* p, int withmask, double windowk, const double* S, double* Wal,
                           double* Waldk, double* Wfold, double* device_ms) {
    if (!k || !x || !Qt || !T || !p || !Wal) return fail("eftb_window_precompute: null argument");
    if (Na < 1 || Na > 3 || Nl < 1 || Nl > 3 || Na > Nl) return fail("eftb_window_precompute: need 1 <= Na <= Nl <= 3 (got Na=%d, Nl=%d)", Na, Nl);
    if (Nk < 1 || nx < 1 || Np < 1 || Nk > 65535) return fail("eftb_window_precompute: bad sizes Nk=%d nx=%d Np=%d", Nk, nx, Np);
    if ((Waldk || Wfold) && !(windowk > 0.0)) return fail("eftb_window_precompute: windowk must be positive");
    if (Wfold && !S) return fail("eftb_window_precompute: Wfold needs the spline matrix S [Np][Nk]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("eftb_window_precompute: no HIP device visible");
    HIPCHK(hipSetDevice(device));
    const size_t R = (size_t)Na * Nl, nW = R * Nk * Np;
    Ledger own;
    auto dalloc = [&](size_t n, double** out) { return own_dev(own, out, n * sizeof(double)); };
    double *dk, *dx, *dQ, *dT, *dp, *dA, *dW, *dWd = nullptr, *dS = nullptr, *dF = nullptr;
    HIPCHK(dalloc(Nk, &dk)); HIPCHK(dalloc(nx, &dx)); HIPCHK(dalloc(R * nx, &dQ)); HIPCHK(dalloc((size_t)Nl * nx * Np, &dT));
    HIPCHK(dalloc(Np, &dp)); HIPCHK(dalloc(R * Nk * nx, &dA)); HIPCHK(dalloc(nW, &dW));
    if (Waldk || Wfold) HIPCHK(dalloc(nW, &dWd));
    if (Wfold) { HIPCHK(dalloc((size_t)Np * Nk, &dS)); HIPCHK(dalloc(R * Nk * Nk, &dF)); }
    HIPCHK(hipMemcpy(dk, k, Nk * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dx, x, nx * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dQ, Qt, R * nx * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dT, T, (size_t)Nl * nx * Np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp, p, Np * sizeof(double), hipMemcpyHostToDevice));
    if (Wfold) HIPCHK(hipMemcpy(dS, S, (size_t)Np * Nk * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipEvent_t ev0, ev1;
    HIPCHK(own_event(own, &ev0));
    HIPCHK(own_event(own, &ev1));
    HIPCHK(hipEventRecord(ev0, 0));
    hipLaunchKernelGGL(window_bessel_kernel, dim3((nx + 255) / 256, Nk), dim3(256), 0, 0, Na, Nl, Nk, nx, dk, dx, dQ, dA);
    for (int l = 0; l < Nl; ++l) {  // rows = (a, k), A_al [Nk][nx] @ T_l [nx][Np]
        GemmDesc g{};
        g.A = dA + (size_t)l * Nk * nx; g.a_group = (long long)Nl * Nk * nx; g.a_row = nx; g.a_seg = 0;
        g.rows = Na * Nk; g.rows_per_group = Nk; g.nseg = 1; g.kseg = nx;
        g.B = dT + (size_t)l * nx * Np; g.ldb = Np; g.ncols = Np;
        g.C = dW + (size_t)l * Nk * Np; g.c_group = (long long)Nl * Nk * Np; g.c_row = Np; g.c_colgroup = 0; g.cols_per_group = Np;
        hipLaunchKernelGGL(gemm_rows_kernel, dim3((g.rows + 63) / 64, (g.ncols + 255) / 256), dim3(256), GEMM_LDS, 0, g);
    }
    if (dWd) hipLaunchKernelGGL(window_maskdp_kernel, dim3((unsigned)((nW + 255) / 256)), dim3(256), 0, 0, (int)R, Nk, Np, dk, dp, withmask, windowk, dW, dWd);
    if (Wfold) {  // rows = (a, l, k), Waldk [.][Np] @ S [Np][Nk]
        GemmDesc g{};
        g.A = dWd; g.a_group = 0; g.a_row = Np; g.a_seg = 0;
        g.rows = (int)(R * Nk); g.rows_per_group = g.rows; g.nseg = 1; g.kseg = Np;
        g.B = dS; g.ldb = Nk; g.ncols = Nk;
        g.C = dF; g.c_group = 0; g.c_row = Nk; g.c_colgroup = 0; g.cols_per_group = Nk;
        hipLaunchKernelGGL(gemm_rows_kernel, dim3((g.rows + 63) / 64, (g.ncols + 255) / 256), dim3(256), GEMM_LDS, 0, g);
    }
    HIPCHK(hipEventRecord(ev1, 0));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    if (device_ms) *device_ms = ms;
    HIPCHK(hipMemcpy(Wal, dW, nW * sizeof(double), hipMemcpyDeviceToHost));
    if (Waldk) HIPCHK(hipMemcpy(Waldk, dWd, nW * sizeof(double), hipMemcpyDeviceToHost));
    if (Wfold) HIPCHK(hipMemcpy(Wfold, dF, R * Nk * Nk * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ draws given as parameter values
// (after every other entry point: the kernels instantiated here are emitted behind the existing ones, whose code and labels stay as they were)
int eftb_set_draw_recipe(eftb_engine* e, int kind, int P, int ng1, int nterms, const eftb_draw_term* terms) {
    static const char* who = "eftb_set_draw_recipe";
    if (e) sub_drain(e);
    if (!e) return fail("%s: null engine", who);
    if (kind != 0 && kind != 1) return fail("%s: kind %d (0: eftb_draws_logp_params, 1: eftb_draws_reduce_params)", who, kind);
    eftb_engine::Recipe& rc = e->recipe[kind];
    if (nterms == 0) {
        rc.set = false;
        return 0;
    }
    if (!terms) return fail("%s: null terms", who);
    if (P < 0 || P > RECIPE_MAXP) return fail("%s: %d parameters, at most %d", who, P, RECIPE_MAXP);
    if (nterms < 0 || nterms > RECIPE_MAXTERMS) return fail("%s: %d terms, at most %d", who, nterms, RECIPE_MAXTERMS);
    if (kind == 0 ? (ng1 < 1 || ng1 > MARG_NG1) : ng1 != 1) return fail("%s: ng1 = %d (kind 0: 1 ... %d, kind 1: 1)", who, ng1, MARG_NG1);
    if (kind == 0 && !e->like_ndata) return fail("%s: the logp recipe belongs to a likelihood: needs eftb_set_likelihood first", who);
    if (kind == 0 && ng1 != e->like_nG + 1) return fail("%s: the recipe has ng1 = %d rows, the likelihood nG + 1 = %d", who, ng1, e->like_nG + 1);
    const int ntr = e->ntr, ncol = e->c.with_nnlo ? NROW + 3 : NROW;
    if (ntr > RECIPE_MAXTR) return fail("%s: %d tracers, a draw recipe takes at most %d", who, ntr, RECIPE_MAXTR);
    for (int t = 0; t < nterms; ++t) {
        const eftb_draw_term& q = terms[t];
        if (q.tracer < 0 || q.tracer >= ntr) return fail("%s: term %d: tracer %d outside [0, %d)", who, t, q.tracer, ntr);
        if (q.row < 0 || q.row >= ng1) return fail("%s: term %d: row %d outside [0, %d)", who, t, q.row, ng1);
        if (q.col < 0 || q.col >= ncol)
            return fail("%s: term %d: column %d outside [0, %d)%s", who, t, q.col, ncol, e->c.with_nnlo ? "" : " (the NNLO columns 24 ... 26 need an engine built with with_nnlo)");
        if (q.fpow < 0 || q.fpow >= RECIPE_FPOW) return fail("%s: term %d: f^%d, powers 0 ... %d", who, t, q.fpow, RECIPE_FPOW - 1);
        for (int ix : {q.i, q.j, q.k})
            if (ix < -1 || ix >= P) return fail("%s: term %d: parameter index %d outside [-1, %d)", who, t, ix, P);
        if (!std::isfinite(q.coef)) return fail("%s: term %d: the coefficient is not finite", who, t);
    }
    // the order the kernels sum in: entries by (row, tracer, column); inside an entry by (fpow, i, j, k) descending indices first, then the
    // coefficient -- independent of the order the terms arrive in
    struct Key {
        int row, tracer, col, fpow, ix[3];
        double coef;
    };
    std::vector<Key> keys(nterms);
    for (int t = 0; t < nterms; ++t) {
        const eftb_draw_term& q = terms[t];
        Key& k = keys[t];
        k.row = q.row; k.tracer = q.tracer; k.col = q.col; k.fpow = q.fpow; k.coef = q.coef;
        k.ix[0] = q.i; k.ix[1] = q.j; k.ix[2] = q.k;
        std::sort(k.ix, k.ix + 3, std::greater<int>());  // (the -1 entries last)
    }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        return std::tie(a.row, a.tracer, a.col, a.fpow, a.ix[0], a.ix[1], a.ix[2], a.coef) < std::tie(b.row, b.tracer, b.col, b.fpow, b.ix[0], b.ix[1], b.ix[2], b.coef);
    });
    std::vector<int> rowstart(ng1 + 1, 0), ent, tstart, pack(nterms), slot((size_t)ntr * (NROW + 3), -1);
    std::vector<double> coef(nterms);
    bool nnlo = false;
    for (int t = 0; t < nterms; ++t) {
        const Key& k = keys[t];
        if (t == 0 || k.row != keys[t - 1].row || k.tracer != keys[t - 1].tracer || k.col != keys[t - 1].col) {
            if (k.row == 0) slot[(size_t)k.tracer * (NROW + 3) + k.col] = (int)ent.size();
            ent.push_back(k.tracer * 32 + k.col);
            tstart.push_back(t);
            ++rowstart[k.row + 1];
        }
        nnlo = nnlo || k.col >= NROW;
        auto ix = [P](int v) { return v < 0 ? P : v; };
        pack[t] = ix(k.ix[0]) | ix(k.ix[1]) << 6 | ix(k.ix[2]) << 12 | (k.tracer * RECIPE_FPOW + k.fpow) << 18;
        coef[t] = k.coef;
    }
    tstart.push_back(nterms);
    for (int g = 0; g < ng1; ++g) rowstart[g + 1] += rowstart[g];
    const int nnz = (int)ent.size();
    // the derivative of the sorted terms (kind 0): one record per (term, distinct theta index p in it) with the coefficient times the
    // multiplicity of p and the two remaining indices; p outermost, the terms in their order: sorted by (p, entry, parent term)
    std::vector<int> pstart, dent, dpack, erow;
    std::vector<double> dcoef;
    if (kind == 0) {
        for (int n = 0, g = 0; n < nnz; ++n) {
            while (n >= rowstart[g + 1]) ++g;
            erow.push_back(g);
        }
        for (int p = 0; p < P; ++p) {
            pstart.push_back((int)dent.size());
            for (int t = 0, n = -1; t < nterms; ++t) {
                if (n + 1 < nnz && tstart[n + 1] == t) ++n;
                const Key& k = keys[t];
                int mult = 0, rest[3] = {-1, -1, -1}, nr = 0;
                for (int q = 0; q < 3; ++q) {
                    if (k.ix[q] == p && mult++ == 0) continue;  // (the first occurrence is the factor differentiated)
                    rest[nr++] = k.ix[q];
                }
                if (!mult) continue;
                auto ix = [P](int v) { return v < 0 ? P : v; };
                dent.push_back(n);
                dpack.push_back(ix(rest[0]) | ix(rest[1]) << 6 | P << 12 | (k.tracer * RECIPE_FPOW + k.fpow) << 18);
                dcoef.push_back(k.coef * mult);
            }
        }
        pstart.push_back((int)dent.size());
    }
    // the second derivative (kind 0): one record per (term, pair p <= q of theta indices in it) with the coefficient times m_p m_q (p < q)
    // or m_p (m_p - 1) (p = q) and the one remaining index; pairs outermost, the terms in their order: sorted by (p, q, entry, parent term)
    std::vector<int> hstart, hent, hpack;
    std::vector<double> hcoef;
    if (kind == 0) {
        for (int p = 0; p < P; ++p)
            for (int q = p; q < P; ++q) {
                hstart.push_back((int)hent.size());
                for (int t = 0, n = -1; t < nterms; ++t) {
                    if (n + 1 < nnz && tstart[n + 1] == t) ++n;
                    const Key& k = keys[t];
                    int mp = 0, mq = 0, rest = -1, takep = 1, takeq = 1;
                    for (int x = 0; x < 3; ++x) {
                        mp += k.ix[x] == p;
                        mq += k.ix[x] == q;
                    }
                    const int mult = p == q ? mp * (mp - 1) : mp * mq;
                    if (!mult) continue;
                    for (int x = 0; x < 3; ++x) {  // (one factor theta_p and one theta_q are differentiated; what is left is at most one index)
                        if (k.ix[x] == p && takep) { takep = 0; continue; }
                        if (k.ix[x] == q && takeq) { takeq = 0; continue; }
                        rest = k.ix[x];
                    }
                    hent.push_back(n);
                    hpack.push_back((rest < 0 ? P : rest) | (k.tracer * RECIPE_FPOW + k.fpow) << 18);
                    hcoef.push_back(k.coef * mult);
                }
            }
        hstart.push_back((int)hent.size());
    }
    std::vector<int> htab;
    for (const std::vector<int>* v : {&hstart, &hent, &hpack}) htab.insert(htab.end(), v->begin(), v->end());
    std::vector<int> dtab;
    for (const std::vector<int>* v : {&pstart, &dent, &dpack, &erow}) dtab.insert(dtab.end(), v->begin(), v->end());
    std::vector<int> tab;
    for (const std::vector<int>* v : {&rowstart, &ent, &tstart, &pack, &slot}) tab.insert(tab.end(), v->begin(), v->end());
    HIPCHK(hipSetDevice(e->c.device));
    HIPCHK(sync_all(e));  // (a params call is synchronous: nothing reads the old tables any more; as eftb_set_likelihood)
    rc.set = false;
    for (void* p : {(void*)rc.coef, (void*)rc.tab, (void*)rc.dcoef, (void*)rc.dtab, (void*)rc.hcoef, (void*)rc.htab}) e->own.release(p);
    rc.coef = nullptr;
    rc.tab = nullptr;
    rc.dcoef = nullptr;
    rc.dtab = nullptr;
    rc.hcoef = nullptr;
    rc.htab = nullptr;
    HIPCHK(own_dev(e->own, &rc.coef, coef.size() * sizeof(double)));
    HIPCHK(own_dev(e->own, &rc.tab, tab.size() * sizeof(int)));
    HIPCHK(hipMemcpy(rc.coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rc.tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    if (kind == 0) {  // (a table without records still holds pstart and erow)
        HIPCHK(own_dev(e->own, &rc.dcoef, std::max<size_t>(1, dcoef.size()) * sizeof(double)));
        HIPCHK(own_dev(e->own, &rc.dtab, dtab.size() * sizeof(int)));
        if (!dcoef.empty()) HIPCHK(hipMemcpy(rc.dcoef, dcoef.data(), dcoef.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(rc.dtab, dtab.data(), dtab.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(own_dev(e->own, &rc.hcoef, std::max<size_t>(1, hcoef.size()) * sizeof(double)));
        HIPCHK(own_dev(e->own, &rc.htab, htab.size() * sizeof(int)));
        if (!hcoef.empty()) HIPCHK(hipMemcpy(rc.hcoef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(rc.htab, htab.data(), htab.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    rc.ndt = (int)dcoef.size();
    rc.nh = (int)hcoef.size();
    rc.P = P; rc.ng1 = ng1; rc.nterms = nterms; rc.nnz = nnz; rc.nnlo = nnlo; rc.ntr_used = ntr;
    rc.set = true;
    return 0;
}

static RecipeTab recipe_tab(const eftb_engine::Recipe& rc) {
    RecipeTab rt{};
    rt.coef = rc.coef;
    rt.rowstart = rc.tab;
    rt.ent = rt.rowstart + rc.ng1 + 1;
    rt.tstart = rt.ent + rc.nnz;
    rt.pack = rt.tstart + rc.nnz + 1;
    rt.slot = rt.pack + rc.nterms;
    rt.P = rc.P;
    rt.nnz = rc.nnz;
    return rt;
}

// the recipe of a params call and its inputs: refusals before anything is copied
static int draws_params_check(eftb_engine* e, const char* who, int kind, int ng1, int C, long long N, const double* theta, const double* f) {
    const eftb_engine::Recipe& rc = e->recipe[kind];
    if (!rc.set) return fail("%s: no draw recipe (eftb_set_draw_recipe kind %d; eftb_set_tracers%s drops it)", who, kind, kind == 0 ? " and eftb_set_likelihood" : "");
    if (rc.ng1 != ng1) return fail("%s: the draw recipe has ng1 = %d rows, the call needs %d", who, rc.ng1, ng1);
    if (rc.ntr_used != e->ntr) return fail("%s: the draw recipe was set for %d tracers, the engine has %d", who, rc.ntr_used, e->ntr);
    if (rc.nnlo && !e->c.with_nnlo) return fail("%s: the draw recipe has NNLO columns, the engine was built without with_nnlo", who);
    for (long long q = 0; q < N * rc.P; ++q)
        if (!std::isfinite(theta[q])) return fail("%s: theta[%lld][%d] is not finite", who, q / rc.P, (int)(q % rc.P));
    for (int q = 0; q < C * e->ntr; ++q)
        if (!std::isfinite(f[q])) return fail("%s: f[%d][%d] is not finite", who, q / e->ntr, q % e->ntr);
    return 0;
}

// theta [N][P] and f [C][ntr] to the device (one buffer: theta, then f)
static int draws_params_upload(eftb_engine* e, int P, int C, long long N, const double* theta, const double* f, const double** dtheta, const double** df) {
    const size_t nt = (size_t)N * P, nf = (size_t)C * e->ntr;
    if (int rc = grow_dev(e, &e->drw_theta, &e->drw_theta_cap, nt + nf)) return rc;
    if (nt) HIPCHK(hipMemcpyAsync(e->drw_theta, theta, nt * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->drw_theta + nt, f, nf * sizeof(double), hipMemcpyHostToDevice, e->stream));
    *dtheta = e->drw_theta;
    *df = e->drw_theta + nt;
    return 0;
}

// the groups of eftb_draws_logp_params_datasets: group g = (walker[g], dataset[g]), every walker below nwalk, every data set below dset_M
struct DrawGroups {
    int nwalk;
    const int32_t *walker, *dataset;
};

// Wg [G][J1][J1] of a groups call, after draws_gram: kept while the template block, the likelihood, the tracers (draw_gen), the data sets
// (dset_gen) and the group table are those it was built from
static int draws_gram_groups(eftb_engine* e, const char* who, int G, int J1, const DrawGroups& gr) {
    if (e->grp_draw_gen == e->draw_gen && e->grp_dset_gen == e->dset_gen && e->grp_tab.size() == 2 * (size_t)G &&
        std::equal(gr.walker, gr.walker + G, e->grp_tab.begin()) && std::equal(gr.dataset, gr.dataset + G, e->grp_tab.begin() + G))
        return 0;
    e->grp_draw_gen = 0;
    char shape[64];
    snprintf(shape, sizeof shape, "G = %d groups with J + 1 = %d columns", G, J1);
    if (int rc = grow_dev(e, &e->drw_Wg, &e->drw_Wg_cap, (size_t)G * J1 * J1, sizeof(double), who, "the Gram matrices", shape)) return rc;
    if (int rc = grow_dev(e, &e->drw_gtab, &e->drw_gtab_cap, 2 * (size_t)G, sizeof(int))) return rc;
    e->grp_tab.assign(gr.walker, gr.walker + G);
    e->grp_tab.insert(e->grp_tab.end(), gr.dataset, gr.dataset + G);
    HIPCHK(hipMemcpyAsync(e->drw_gtab, e->grp_tab.data(), 2 * (size_t)G * sizeof(int), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(draws_gram_groups_kernel<256>, dim3(G), dim3(256), 0, e->stream, e->like_ndata, J1, e->drw_gtab, e->drw_gtab + G, e->drw_A, e->drw_U,
                       e->drw_W, e->dset_D, e->dset_Ud, e->drw_Wg);
    if (int rc = launched(who)) return rc;
    e->grp_draw_gen = e->draw_gen;
    e->grp_dset_gen = e->dset_gen;
    return 0;
}

// What the params calls do between "the shape is known" and their launch: draws_logp_begin, Wg of a groups call (the kernels read it where they
// read W_c), theta and f on the device, the launch geometry and the recipe's table
struct DrawRun {
    const double *W, *theta, *f;
    dim3 grid, block;
    RecipeTab rt;
};
static int draws_params_begin(eftb_engine* e, const char* who, int C, long long N, long long maxcnt, const DrawShape& sh, const int64_t* offsets,
                              const double* theta, const double* f, const DrawGroups* gr, DrawRun* run) {
    if (int rc = draws_logp_begin(e, who, C, N, sh.J1, offsets, gr ? gr->nwalk : -1)) return rc;
    if (gr)
        if (int rc = draws_gram_groups(e, who, C, sh.J1, *gr)) return rc;
    run->W = gr ? e->drw_Wg : e->drw_W;
    if (int rc = draws_params_upload(e, e->recipe[0].P, C, N, theta, f, &run->theta, &run->f)) return rc;
    run->grid = dim3(C, draw_shares(maxcnt, sh.nw, C));
    run->block = dim3(64 * sh.nw);
    run->rt = recipe_tab(e->recipe[0]);
    return 0;
}

// eftb_draws_logp_params (grad == nullptr: the forward kernel and its LDS layout), eftb_draws_logp_grad_params and eftb_draws_logp_hess_params
// (hess != nullptr, with grad: the Hessian kernel and its LDS layout).  gr (eftb_draws_logp_params_datasets): C counts the groups, offsets and
// f [C][ntr] are per group, and the kernels read Wg where they read W_c
static int draws_logp_params_impl(eftb_engine* e, const char* who, int C, long long N, const int64_t* offsets, const double* theta, const double* f,
                                  double* logp, double* grad, double* fullchi2, double* best, double* hess = nullptr, const DrawGroups* gr = nullptr) {
    long long maxcnt = 0;
    if (int rc = draws_logp_check(e, who, C, N, offsets, &maxcnt, gr ? "group" : "walker", gr ? gr->nwalk : -1)) return rc;
    const int ntr = e->ntr, nG = e->like_nG;
    if (int rc = draws_params_check(e, who, 0, nG + 1, C, N, theta, f)) return rc;
    const eftb_engine::Recipe& rcp = e->recipe[0];
    const int P = rcp.P;
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, hess ? DRAW_HESS : grad ? DRAW_GRAD : DRAW_PARAMS, &rcp, &sh)) return rc;
    if (!sh.nw) {
        if (!hess) return draws_no_fit(who, sh.J1);
        return fail("%s: the Hessian of P = %d parameters with nG = %d and J + 1 = %d columns does not fit the LDS (%zu bytes per workgroup and %zu per wave)",
                    who, P, nG, sh.J1, sh.L.bytes_wg(), sh.L.bytes_wave());
    }
    if (N == 0) return 0;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, maxcnt, sh, offsets, theta, f, gr, &run)) return rc;
    if (grad)
        if (int rc = grow_dev(e, &e->drw_grad, &e->drw_grad_cap, std::max<size_t>(1, (size_t)N * P))) return rc;
    if (hess)
        if (int rc = grow_dev(e, &e->drw_hess, &e->drw_hess_cap, std::max<size_t>(1, (size_t)N * P * P))) return rc;
    hipStream_t st = e->stream;
    const int J1 = sh.J1;
    RecipeGradTab gt{};
    gt.dcoef = rcp.dcoef;
    gt.pstart = rcp.dtab;
    gt.dent = gt.pstart + P + 1;
    gt.dpack = gt.dent + rcp.ndt;
    gt.erow = gt.dpack + rcp.ndt;
    while ((1 << gt.lgP2) < P) ++gt.lgP2;
    if (hess) {
        RecipeHessTab ht{};
        ht.npair = P * (P + 1) / 2;
        ht.ndt = rcp.ndt;
        ht.hcoef = rcp.hcoef;
        ht.hstart = rcp.htab;
        ht.hent = ht.hstart + ht.npair + 1;
        ht.hpack = ht.hent + rcp.nh;
        while ((1 << ht.lgPP) < std::min(ht.npair, 64)) ++ht.lgPP;
        launch_two(draws_logp_hess_params_kernel<false>, draws_logp_hess_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, J1, e->jeffreys, run.rt, gt,
                   ht, e->drw_off, run.theta, run.f, run.W, e->like_mu, e->like_sinv, e->drw_out, e->drw_grad, e->drw_hess);
    } else if (grad)
        launch_two(draws_logp_grad_params_kernel<false>, draws_logp_grad_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, J1, e->jeffreys, run.rt, gt,
                   e->drw_off, run.theta, run.f, run.W, e->like_mu, e->like_sinv, e->drw_out, e->drw_grad);
    else
        launch_two(draws_logp_params_kernel<false>, draws_logp_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, J1, e->jeffreys, run.rt, e->drw_off,
                   run.theta, run.f, run.W, e->like_mu, e->like_sinv, e->drw_out);
    if (int rc = launched(who)) return rc;
    if (grad && P) HIPCHK(hipMemcpyAsync(grad, e->drw_grad, (size_t)N * P * sizeof(double), hipMemcpyDeviceToHost, st));
    if (hess && P) HIPCHK(hipMemcpyAsync(hess, e->drw_hess, (size_t)N * P * P * sizeof(double), hipMemcpyDeviceToHost, st));
    return draws_records(e, N, logp, fullchi2, best);
}

int eftb_draws_logp_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                           double* fullchi2, double* best) {
    static const char* who = "eftb_draws_logp_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta || !logp))) return fail("%s: null argument", who);
    return draws_logp_params_impl(e, who, C, N, offsets, theta, f, logp, nullptr, fullchi2, best);
}

// draws_reduce_kernel on the coefficient rows bias [n][ntr][24] (with NNLO, biasn [n][ntr][3]) of the draws that off [C + 1] deals to the walkers
static int launch_draws_reduce(eftb_engine* e, const char* who, int C, long long maxcnt, const long long* off, const double* bias, const double* biasn,
                               double* plk) {
    const eftb_config& c = e->c;
    const int ntr = e->ntr, nl = e->cur_nl, nx = e->cur_nx, xtiles = (nx + 63) / 64, shares = draw_shares(maxcnt, 4, (long long)C * ntr * nl * xtiles);
    hipLaunchKernelGGL(draws_reduce_kernel, dim3(xtiles * shares, ntr * nl, C), dim3(256), 0, e->stream, nx, nl, ntr, reduce_msplit(c), xtiles, off, bias,
                       e->buf[EFTB_B_TEMPL], c.with_nnlo ? biasn : nullptr, c.with_nnlo ? e->buf[EFTB_B_TEMPLN] : nullptr, plk);
    return launched(who);
}

// eftb_draws_reduce (the caller's bias and bias_nnlo) and eftb_draws_reduce_params (f != nullptr: the rows of recipe 1 at theta and f)
static int draws_reduce_impl(eftb_engine* e, const char* who, int C, long long N, const int64_t* offsets, const double* bias, const double* bias_nnlo,
                             const double* theta, const double* f, double* plk) {
    long long maxcnt = 0;
    if (int rc = draws_check(e, who, C, N, offsets, &maxcnt)) return rc;
    const eftb_config& c = e->c;
    if (f) {
        if (int rc = draws_params_check(e, who, 1, 1, C, N, theta, f)) return rc;
    } else if (bias_nnlo && !c.with_nnlo) return fail("%s: bias_nnlo needs an engine built with with_nnlo", who);
    if (N == 0) return 0;
    const int ntr = e->ntr;
    HIPCHK(hipSetDevice(c.device));
    hipStream_t st = e->stream;
    join_back(e);
    const size_t bn = (size_t)N * ntr * NROW, bnn = (size_t)N * ntr * 3, pn = (size_t)N * ntr * e->cur_nl * e->cur_nx;
    if (int rc = grow_dev(e, &e->drw_off, &e->drw_off_cap, (size_t)C + 1, sizeof(long long))) return rc;
    if (int rc = grow_dev(e, &e->drw_in, &e->drw_in_cap, bn)) return rc;
    if (int rc = grow_dev(e, &e->drw_out, &e->drw_out_cap, pn)) return rc;
    if (c.with_nnlo)
        if (int rc = grow_dev(e, &e->drw_inn, &e->drw_inn_cap, bnn)) return rc;
    HIPCHK(hipMemcpyAsync(e->drw_off, offsets, ((size_t)C + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (f) {
        const eftb_engine::Recipe& rcp = e->recipe[1];
        const double *dtheta = nullptr, *df = nullptr;
        if (int rc = draws_params_upload(e, rcp.P, C, N, theta, f, &dtheta, &df)) return rc;
        const dim3 rgrid(C, draw_shares(maxcnt, 4, C));
        if (c.with_nnlo) hipLaunchKernelGGL(draws_recipe_rows_kernel<true>, rgrid, dim3(256), 0, st, ntr, recipe_tab(rcp), e->drw_off, dtheta, df, e->drw_in, e->drw_inn);
        else hipLaunchKernelGGL(draws_recipe_rows_kernel<false>, rgrid, dim3(256), 0, st, ntr, recipe_tab(rcp), e->drw_off, dtheta, df, e->drw_in, nullptr);
    } else {
        HIPCHK(hipMemcpyAsync(e->drw_in, bias, bn * sizeof(double), hipMemcpyHostToDevice, st));
        if (c.with_nnlo) {  // (no bias_nnlo: zeros, as the REDUCE stage of eftb_eval_batch)
            if (bias_nnlo) HIPCHK(hipMemcpyAsync(e->drw_inn, bias_nnlo, bnn * sizeof(double), hipMemcpyHostToDevice, st));
            else HIPCHK(hipMemsetAsync(e->drw_inn, 0, bnn * sizeof(double), st));
        }
    }
    if (int rc = launch_draws_reduce(e, who, C, maxcnt, e->drw_off, e->drw_in, e->drw_inn, e->drw_out)) return rc;
    HIPCHK(hipMemcpyAsync(plk, e->drw_out, pn * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int eftb_draws_reduce(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* bias, const double* bias_nnlo, double* plk) {
    static const char* who = "eftb_draws_reduce";
    if (e) sub_drain(e);
    if (!e || !offsets || (N > 0 && (!bias || !plk))) return fail("%s: null argument", who);
    return draws_reduce_impl(e, who, C, N, offsets, bias, bias_nnlo, nullptr, nullptr, plk);
}

int eftb_draws_reduce_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* plk) {
    static const char* who = "eftb_draws_reduce_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta || !plk))) return fail("%s: null argument", who);
    return draws_reduce_impl(e, who, C, N, offsets, nullptr, nullptr, theta, f, plk);
}

// ------------------------------------------------------------------------------------------------ d ln P / d theta of params draws
int eftb_draws_logp_grad_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                                double* grad, double* fullchi2, double* best) {
    static const char* who = "eftb_draws_logp_grad_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta || !logp))) return fail("%s: null argument", who);
    if (!grad) return fail("%s: grad == NULL (eftb_draws_logp_params is the call without the gradient)", who);
    return draws_logp_params_impl(e, who, C, N, offsets, theta, f, logp, grad, fullchi2, best);
}

// ------------------------------------------------------------------------------------------------ d2 ln P / d theta d theta of params draws
int eftb_draws_logp_hess_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                                double* grad, double* hess, double* fullchi2, double* best) {
    static const char* who = "eftb_draws_logp_hess_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta || !logp))) return fail("%s: null argument", who);
    if (!grad) return fail("%s: grad == NULL (the Hessian call returns the gradient too)", who);
    if (!hess) return fail("%s: hess == NULL (eftb_draws_logp_grad_params is the call without the Hessian)", who);
    return draws_logp_params_impl(e, who, C, N, offsets, theta, f, logp, grad, fullchi2, best, hess);
}

int eftb_set_likelihood_datasets(eftb_engine* e, int M, const double* data) {
    static const char* who = "eftb_set_likelihood_datasets";
    if (e) sub_drain(e);
    if (!e) return fail("%s: null engine", who);
    if (M == 0) {
        e->dset_M = 0;
        ++e->dset_gen;
        return 0;
    }
    if (M < 0) return fail("%s: %d data sets", who, M);
    if (!data) return fail("%s: null data", who);
    if (!e->like_ndata) return fail("%s: the data sets share a likelihood's index, covariance and priors: needs eftb_set_likelihood first", who);
    const int nd = e->like_ndata;
    for (size_t q = 0; q < (size_t)M * nd; ++q)
        if (!std::isfinite(data[q])) return fail("%s: data[%zu][%zu] is not finite", who, q / nd, q % nd);
    HIPCHK(hipSetDevice(e->c.device));
    join_back(e);
    e->dset_M = 0;
    ++e->dset_gen;
    if (int rc = grow_dev(e, &e->dset_D, &e->dset_D_cap, (size_t)M * nd)) return rc;
    if (int rc = grow_dev(e, &e->dset_Ud, &e->dset_Ud_cap, (size_t)M * nd)) return rc;
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(e->dset_D, data, (size_t)M * nd * sizeof(double), hipMemcpyHostToDevice, st));
    launch_times_invcov(e, st, e->dset_D, M, e->dset_Ud);  // Ud = D C^-1, as draws_gram multiplies A: a row of -D there is the exact negation of its row here
    if (int rc = launched(who)) return rc;
    HIPCHK(hipStreamSynchronize(st));  // (the caller's array is free again)
    e->dset_M = M;
    return 0;
}

// the group table of a data-sets call (gr->walker and gr->dataset [G] of the caller): refusals, gr->nwalk, and f [C][ntr] expanded to grp_f [G][ntr]
static int draws_groups_check(eftb_engine* e, const char* who, int C, int G, const double* f, DrawGroups* gr) {
    const int32_t *walker = gr->walker, *dataset = gr->dataset;
    if (!e->like_ndata) return fail("%s: needs eftb_set_likelihood", who);
    if (!e->dset_M) return fail("%s: no data sets (eftb_set_likelihood_datasets; eftb_set_likelihood and eftb_set_tracers drop them)", who);
    if (C < 1) return fail("%s: %d walkers", who, C);
    if (G < 1) return fail("%s: %d groups", who, G);
    const int ntr = e->ntr;
    const size_t per = (size_t)e->cur_nl * NROW * e->cur_nx, have = per ? e->templ_elems / per : 0;
    gr->nwalk = 0;
    for (int g = 0; g < G; ++g) {
        if (walker[g] < 0 || walker[g] >= C) return fail("%s: walker[%d] = %d outside [0, %d)", who, g, walker[g], C);
        if (dataset[g] < 0 || dataset[g] >= e->dset_M) return fail("%s: dataset[%d] = %d outside [0, %d)", who, g, dataset[g], e->dset_M);
        if (e->templ_ok && ((size_t)walker[g] + 1) * ntr > have)
            return fail("%s: walker[%d] = %d with %d tracers, but the template block holds %zu entries [%d][24][%d]", who, g, walker[g], ntr, have, e->cur_nl,
                        e->cur_nx);
        gr->nwalk = std::max(gr->nwalk, walker[g] + 1);
    }
    for (int q = 0; q < C * ntr; ++q)
        if (!std::isfinite(f[q])) return fail("%s: f[%d][%d] is not finite", who, q / ntr, q % ntr);
    e->grp_f.resize((size_t)G * ntr);  // f per group: the draw kernels read f [blockIdx.x][ntr]
    for (int g = 0; g < G; ++g) std::copy(f + (size_t)walker[g] * ntr, f + ((size_t)walker[g] + 1) * ntr, e->grp_f.begin() + (size_t)g * ntr);
    return 0;
}

int eftb_draws_logp_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, const int64_t* offsets,
                                    const double* theta, const double* f, double* logp, double* grad, double* hess, double* fullchi2, double* best) {
    static const char* who = "eftb_draws_logp_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || (N > 0 && (!theta || !logp))) return fail("%s: null argument", who);
    if (hess && !grad) return fail("%s: hess needs grad (the Hessian kernel returns the gradient too)", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_logp_params_impl(e, who, G, N, offsets, theta, e->grp_f.data(), logp, grad, fullchi2, best, hess, &gr);
}

// ------------------------------------------------------------------------------------------------ samples of the marginalised parameters
// eftb_draws_sample_params and eftb_draws_sample_params_datasets (gr; C counts the groups, offsets and f [C][ntr] are per group, no plk): the
// checks, W_c, uploads and records of draws_logp_params_impl around draws_sample_params_kernel, then draws_reduce_kernel on the [N S]
// coefficient rows where plk is asked for
static int draws_sample_params_impl(eftb_engine* e, const char* who, int C, long long N, int S, const int64_t* offsets, const double* theta, const double* f,
                                    const double* z, double* logp, double* fullchi2, double* best, double* bsamp, double* chi2samp, double* coef,
                                    double* coefn, double* plk, const DrawGroups* gr = nullptr) {
    long long maxcnt = 0;
    if (int rc = draws_logp_check(e, who, C, N, offsets, &maxcnt, gr ? "group" : "walker", gr ? gr->nwalk : -1)) return rc;
    const eftb_config& c = e->c;
    const int ntr = e->ntr, nG = e->like_nG;
    if (S < 1) return fail("%s: S = %d samples per draw, at least 1", who, S);
    if (coefn && !c.with_nnlo) return fail("%s: coefn needs an engine built with with_nnlo", who);
    if (int rc = draws_params_check(e, who, 0, nG + 1, C, N, theta, f)) return rc;
    for (long long q = 0; q < N * S * nG; ++q)
        if (!std::isfinite(z[q])) return fail("%s: z[%lld][%d][%d] is not finite", who, q / ((long long)S * nG), (int)(q / nG % S), (int)(q % nG));
    // (plk: draws_logp_check has held the block to the likelihood's [nl][24][nx] and to its walkers x tracers entries, all eftb_draws_reduce asks)
    const eftb_engine::Recipe& rcp = e->recipe[0];
    const int P = rcp.P;
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_SAMPLE, &rcp, &sh)) return rc;
    // Reachable at one shape only: five tracers (J + 1 = 121), nG = 24 and a recipe of at least 1001 entries (147816 + 16 nnzp bytes
    // at one wave, nnzp the entry count rounded up to even, against 163840); tests/test_gpu_draw_synthetic.py goes there.
    if (!sh.nw) return fail("%s: the samples of nG = %d parameters with J + 1 = %d columns do not fit the LDS (S = %d, %d samples at a time)", who, nG, sh.J1, S, ADJ_KB);
    if (N == 0) return 0;
    const bool want_coef = coef || coefn || plk, nn = c.with_nnlo;
    const int nl = e->cur_nl, nx = e->cur_nx;
    const size_t ns = (size_t)N * S;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, maxcnt, sh, offsets, theta, f, gr, &run)) return rc;
    char shape[96];
    snprintf(shape, sizeof shape, "N = %lld draws x S = %d samples with nG = %d", N, S, nG);
    auto grow = [&](auto* pp, size_t* cap, size_t n, const char* what, size_t elem = sizeof(double)) { return grow_dev(e, pp, cap, n, elem, who, what, shape); };
    if (int rc = grow(&e->smp_z, &e->smp_z_cap, std::max<size_t>(1, ns * nG), "z")) return rc;
    if (int rc = grow(&e->smp_b, &e->smp_b_cap, std::max<size_t>(1, ns * nG), "the samples")) return rc;
    if (int rc = grow(&e->smp_chi2, &e->smp_chi2_cap, ns, "chi2 of the samples")) return rc;
    if (want_coef) {
        if (int rc = grow(&e->smp_coef, &e->smp_coef_cap, ns * ntr * NROW, "the coefficient rows")) return rc;
        if (nn)
            if (int rc = grow(&e->smp_coefn, &e->smp_coefn_cap, ns * ntr * 3, "the NNLO coefficient rows")) return rc;
    }
    if (plk) {
        if (int rc = grow(&e->smp_plk, &e->smp_plk_cap, ns * ntr * nl * nx, "P_l of the samples")) return rc;
        if (int rc = grow(&e->smp_off, &e->smp_off_cap, (size_t)C + 1, "the offsets", sizeof(long long))) return rc;
    }
    hipStream_t st = e->stream;
    if (nG) HIPCHK(hipMemcpyAsync(e->smp_z, z, ns * nG * sizeof(double), hipMemcpyHostToDevice, st));
    const int* erow = rcp.dtab + P + 1 + 2 * rcp.ndt;  // (RecipeGradTab: pstart | dent | dpack | erow)
    double* dcoef = want_coef ? e->smp_coef : nullptr;
    double* dcoefn = want_coef && nn ? e->smp_coefn : nullptr;
    launch_two(draws_sample_params_kernel<false>, draws_sample_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, sh.J1, e->jeffreys, S, run.rt, erow,
               e->drw_off, run.theta, run.f, run.W, e->like_mu, e->like_sinv, e->smp_z, e->drw_out, e->smp_b, e->smp_chi2, dcoef, dcoefn);
    if (int rc = launched(who)) return rc;
    if (plk) {  // the launch of eftb_draws_reduce on N S draws with offsets S
        e->smp_off_host.resize((size_t)C + 1);
        for (int w = 0; w <= C; ++w) e->smp_off_host[w] = (long long)offsets[w] * S;
        HIPCHK(hipMemcpyAsync(e->smp_off, e->smp_off_host.data(), ((size_t)C + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
        if (int rc = launch_draws_reduce(e, who, C, maxcnt * S, e->smp_off, e->smp_coef, e->smp_coefn, e->smp_plk)) return rc;
        HIPCHK(hipMemcpyAsync(plk, e->smp_plk, ns * ntr * nl * nx * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (nG) HIPCHK(hipMemcpyAsync(bsamp, e->smp_b, ns * nG * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(chi2samp, e->smp_chi2, ns * sizeof(double), hipMemcpyDeviceToHost, st));
    if (coef) HIPCHK(hipMemcpyAsync(coef, e->smp_coef, ns * ntr * NROW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (coefn) HIPCHK(hipMemcpyAsync(coefn, e->smp_coefn, ns * ntr * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    return draws_records(e, N, logp, fullchi2, best);
}

int eftb_draws_sample_params(eftb_engine* e, int C, long long N, int S, const int64_t* offsets, const double* theta, const double* f, const double* z,
                             double* logp, double* fullchi2, double* best, double* bsamp, double* chi2samp, double* coef, double* coefn, double* plk) {
    static const char* who = "eftb_draws_sample_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta || !z || !logp || !bsamp || !chi2samp))) return fail("%s: null argument", who);
    return draws_sample_params_impl(e, who, C, N, S, offsets, theta, f, z, logp, fullchi2, best, bsamp, chi2samp, coef, coefn, plk);
}

int eftb_draws_sample_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int S, const int64_t* offsets,
                                      const double* theta, const double* f, const double* z, double* logp, double* fullchi2, double* best, double* bsamp,
                                      double* chi2samp, double* coef, double* coefn) {
    static const char* who = "eftb_draws_sample_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || (N > 0 && (!theta || !z || !logp || !bsamp || !chi2samp))) return fail("%s: null argument", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_sample_params_impl(e, who, G, N, S, offsets, theta, e->grp_f.data(), z, logp, fullchi2, best, bsamp, chi2samp, coef, coefn, nullptr, &gr);
}

// ------------------------------------------------------------------------------------------------ Metropolis chains over the draw parameters
// steps of a chain per launch: no launch's duration grows with the caller's T, and one slice of step and lnu is resident at a time.  An
// evaluation costs tens of microseconds per wave, so 256 steps keep a launch in the milliseconds and spend one evaluation in 256 on the
// record of the launch's starting theta
constexpr int CHAIN_STEPS = 256;

// what the chain calls refuse in their own arguments, after draws_params_check: no parameter, T, thin (at least thin_min), step, lnu, the prior
// on theta and a theta0 outside the box; pri [CHAIN_PRI] = lower | upper | loc | sinv is the table their kernels read.  step and lnu NULL
// (the ensemble call): the caller checks its own moves behind this
static int chain_args_check(const char* who, int P, long long N, int T, int thin, int thin_min, const double* theta0, const double* step, const double* lnu,
                            const double* lower, const double* upper, const double* ploc, const double* pscale, double* pri, const char* step_name = "step") {
    if (P < 1) return fail("%s: the draw recipe has no parameters to move", who);
    if (T < 1) return fail("%s: T = %d steps, at least 1", who, T);
    if (thin < thin_min || thin > T) return fail("%s: thin = %d outside [%d, T = %d]", who, thin, thin_min, T);
    const long long TP = (long long)T * P;
    for (long long q = 0; step && q < N * TP; ++q)
        if (!std::isfinite(step[q])) return fail("%s: %s[%lld][%lld][%d] is not finite", who, step_name, q / TP, q / P % T, (int)(q % P));
    for (long long q = 0; lnu && q < N * T; ++q)
        if (!(lnu[q] <= 0.0)) return fail("%s: lnu[%lld][%lld] = %g is not the logarithm of a uniform in [0, 1]", who, q / T, q % T, lnu[q]);
    for (int p = 0; p < P; ++p) {
        const double lo = lower ? lower[p] : -INFINITY, hi = upper ? upper[p] : INFINITY, sc = pscale ? pscale[p] : INFINITY;
        const double mu = ploc ? ploc[p] : 0.0;
        if (lo != lo || hi != hi) return fail("%s: a bound of parameter %d is NaN", who, p);
        if (lo > hi) return fail("%s: lower[%d] = %g > upper[%d] = %g", who, p, lo, p, hi);
        if (!(sc > 0.0)) return fail("%s: prior_scale[%d] = %g, not > 0", who, p, sc);
        if (std::isfinite(sc) && !std::isfinite(mu)) return fail("%s: prior_loc[%d] is not finite", who, p);
        pri[p] = lo;
        pri[RECIPE_MAXP + p] = hi;
        pri[2 * RECIPE_MAXP + p] = std::isfinite(sc) ? mu : 0.0;
        pri[3 * RECIPE_MAXP + p] = 1.0 / sc;  // (inf: 0, the parameter is skipped)
    }
    for (int p = P; p < RECIPE_MAXP; ++p) pri[p] = pri[RECIPE_MAXP + p] = pri[2 * RECIPE_MAXP + p] = pri[3 * RECIPE_MAXP + p] = 0.0;
    for (long long q = 0; q < N * P; ++q)
        if (!(theta0[q] >= pri[q % P] && theta0[q] <= pri[RECIPE_MAXP + q % P]))
            return fail("%s: theta0[%lld][%d] = %g outside [%g, %g]", who, q / P, (int)(q % P), theta0[q], pri[q % P], pri[RECIPE_MAXP + q % P]);
    return 0;
}

// What the four sampler calls (chains, tempering, HMC, dragging) share on the host.  Each of them reads: chain_front, its own checks, its shape,
// chain_buffers, its own buffers and one-time uploads, chain_run around its own launch, chain_fetch, its own outputs, chain_end
struct ChainCall {
    eftb_engine* e;
    const char* who;
    long long N, maxcnt;    // chains; the most of them one walker (group, pair) owns
    int T, thin, P, nG;
    int per_launch, width;  // steps (trajectories) of a launch; doubles of a stored record: MARG_OUT, or two of them for a pair of walkers
    int mw;                 // doubles of a chain's moves per step: P, or 1 for the stretch factors of the ensemble call
    int K, kstride, Tmax;   // stored states of a chain in the call, at most in one launch, and the steps of the longest launch
    char shape[112];        // the size of the call, for a refused allocation
    double pri[CHAIN_PRI];  // lower | upper | loc | sinv
};
struct ChainRecords {  // where a walker's records go, slot by slot through draws_unpack
    double *logp, *fullchi2, *best;
};
using ChainLaunch = std::function<int(int t0, int Tc, int kc)>;       // this launch's own uploads, then launch_two with the sampler's kernel
using ChainMore = std::function<int(int t0, int Tc, bool landed)>;  // more to bring back behind a launch: enqueue it, then (landed) hand it out

// the refusals no sampler words itself, in the order of the draw calls: C owners (unit; the block must hold nwalk walkers) of the N chains,
// f [Cf][ntr], then chain_args_check on the moves (step or mom) -> maxcnt, P, nG and pri
static int chain_front(ChainCall* c, int C, const char* unit, int nwalk, int Cf, int thin_min, const int64_t* offsets, const double* theta0, const double* f,
                       const double* moves, const double* lnu, const double* lower, const double* upper, const double* ploc, const double* pscale,
                       const char* moves_name = "step") {
    eftb_engine* e = c->e;
    if (int rc = draws_logp_check(e, c->who, C, c->N, offsets, &c->maxcnt, unit, nwalk)) return rc;
    c->nG = e->like_nG;
    if (int rc = draws_params_check(e, c->who, 0, c->nG + 1, Cf, c->N, theta0, f)) return rc;
    c->P = e->recipe[0].P;
    return chain_args_check(c->who, c->P, c->N, c->T, c->thin, thin_min, theta0, moves, lnu, lower, upper, ploc, pscale, c->pri, moves_name);
}

static int chain_grow(const ChainCall& c, void* pp, size_t* cap, size_t n, const char* what, size_t elem = sizeof(double)) {
    return grow_dev(c.e, pp, cap, n, elem, c.who, what, c.shape);
}

// the split into launches of per_launch steps and the buffers every sampler has, records of `width` doubles, moves of `mw` doubles per chain and step (every caller says which: P, or 1 for
// the ensemble call's stretch factors); `moves` and `unit` are the caller's words for a refused allocation.  thin = 0 (dragging alone allows it) stores nothing
static int chain_buffers(ChainCall& c, int per_launch, int width, int mw, const char* moves, const char* unit) {
    eftb_engine* e = c.e;
    c.per_launch = per_launch;
    c.width = width;
    c.mw = mw;
    c.K = c.thin ? c.T / c.thin : 0;
    c.kstride = c.thin ? std::max(1, std::min(c.K, per_launch / c.thin + 1)) : 1;
    c.Tmax = std::min(c.T, per_launch);
    snprintf(c.shape, sizeof c.shape, "N = %lld chains x T = %d %s with P = %d parameters", c.N, c.T, unit, c.P);
    const size_t N = (size_t)c.N;
    if (int rc = chain_grow(c, &e->chn_step, &e->chn_step_cap, N * c.Tmax * c.mw, moves)) return rc;
    if (int rc = chain_grow(c, &e->chn_lnu, &e->chn_lnu_cap, N * c.Tmax, "lnu")) return rc;
    if (int rc = chain_grow(c, &e->chn_pri, &e->chn_pri_cap, CHAIN_PRI, "the prior table")) return rc;
    if (int rc = chain_grow(c, &e->chn_nacc, &e->chn_nacc_cap, N, "the accept counts", sizeof(long long))) return rc;
    if (int rc = chain_grow(c, &e->chn_chain, &e->chn_chain_cap, N * c.kstride * c.P, "the stored states")) return rc;
    return chain_grow(c, &e->chn_rec, &e->chn_rec_cap, N * c.kstride * width, "the stored records");
}

// The prior table and the zeroed accept counts (behind the caller's own one-time uploads), then one launch per per_launch steps.  (The moves
// are c.mw doubles per step: P for the four calls that add increments or momenta, which enqueue what they always did.)  Between the
// launches theta and the accept counts stay on the device; the states and records a launch stored come back behind it, into chain [N][K][P] and,
// one ChainRecords per MARG_OUT of the width, into slot k of `slots` per chain.  A launch that stored nothing is not waited for, unless `more`
// brings something back behind every launch
static int chain_run(const ChainCall& c, const double* moves, const double* lnu, double* chain, const ChainRecords* rec, int slots, const ChainLaunch& launch,
                     const ChainMore& more = nullptr) {
    eftb_engine* e = c.e;
    const size_t N = (size_t)c.N, P = (size_t)c.P, W = (size_t)c.width, T = (size_t)c.T, K = (size_t)c.K, kstride = (size_t)c.kstride, M = (size_t)c.mw;
    const int nG = c.nG, thin = c.thin;
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(e->chn_pri, c.pri, sizeof(c.pri), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(e->chn_nacc, 0, N * sizeof(long long), st));
    e->chn_host_chain.resize(N * kstride * P);
    e->chn_host_rec.resize(N * kstride * W);
    const double *hchain = e->chn_host_chain.data(), *hrec = e->chn_host_rec.data();
    for (int t0 = 0; t0 < c.T; t0 += c.per_launch) {
        const int Tc = std::min(c.per_launch, c.T - t0), k0 = thin ? t0 / thin : 0, kc = thin ? (t0 + Tc) / thin - k0 : 0;
        // this launch's steps of every chain: rows of Tc M (Tc) doubles out of the caller's rows of T M (T), M = P but for the ensemble call
        HIPCHK(hipMemcpy2DAsync(e->chn_step, Tc * M * sizeof(double), moves + t0 * M, T * M * sizeof(double), Tc * M * sizeof(double), N,
                                hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpy2DAsync(e->chn_lnu, Tc * sizeof(double), lnu + t0, T * sizeof(double), Tc * sizeof(double), N, hipMemcpyHostToDevice, st));
        if (int rc = launch(t0, Tc, kc)) return rc;
        if (int rc = launched(c.who)) return rc;
        if (!kc && !more) continue;
        if (kc) {
            HIPCHK(hipMemcpyAsync(e->chn_host_chain.data(), e->chn_chain, N * kstride * P * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(e->chn_host_rec.data(), e->chn_rec, N * kstride * W * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (more)
            if (int rc = more(t0, Tc, false)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        for (size_t n = 0; n < N; ++n)
            for (int k = 0; k < kc; ++k) {
                const size_t from = n * kstride + k;
                std::copy_n(hchain + from * P, P, chain + (n * K + k0 + k) * P);
                for (size_t r = 0; r * MARG_OUT < W; ++r)
                    draws_unpack(hrec + from * W + r * MARG_OUT, nG, n * slots + k0 + k, rec[r].logp, rec[r].fullchi2, rec[r].best);
            }
        if (more)
            if (int rc = more(t0, Tc, true)) return rc;
    }
    return 0;
}

// the end of a call: `last` and the accept counts are enqueued, the caller enqueues its own outputs behind them, and chain_end waits for all
// of it and widens the counts
static int chain_fetch(const ChainCall& c, double* last) {
    eftb_engine* e = c.e;
    e->chn_host_nacc.resize((size_t)c.N);
    HIPCHK(hipMemcpyAsync(last, e->drw_theta, (size_t)c.N * c.P * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(e->chn_host_nacc.data(), e->chn_nacc, (size_t)c.N * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    return 0;
}
static int chain_end(const ChainCall& c, int64_t* naccept) {
    HIPCHK(hipStreamSynchronize(c.e->stream));
    for (long long n = 0; n < c.N; ++n) naccept[n] = c.e->chn_host_nacc[n];
    return 0;
}

// eftb_draws_chain_params and eftb_draws_chain_params_datasets (gr; C counts the groups, offsets and f [C][ntr] are per group): the checks, W_c
// and uploads of draws_logp_params_impl, then draws_chain_params_kernel once per CHAIN_STEPS steps
static int draws_chain_params_impl(eftb_engine* e, const char* who, int C, long long N, int T, int thin, const int64_t* offsets, const double* theta0,
                                   const double* f, const double* step, const double* lnu, const double* lower, const double* upper, const double* ploc,
                                   const double* pscale, double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept,
                                   const DrawGroups* gr = nullptr) {
    ChainCall c{e, who, N, 0, T, thin};
    if (int rc = chain_front(&c, C, gr ? "group" : "walker", gr ? gr->nwalk : -1, C, 1, offsets, theta0, f, step, lnu, lower, upper, ploc, pscale)) return rc;
    const int ntr = e->ntr, nG = c.nG;
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_CHAIN, &e->recipe[0], &sh)) return rc;
    // Unreachable: the largest shape there is (J + 1 = 121, nG = 24, 1024 recipe entries) takes 161288 of the 163840 bytes at one wave.
    if (!sh.nw) return fail("%s: the chains of P = %d parameters with nG = %d and J + 1 = %d columns do not fit the LDS", who, c.P, nG, sh.J1);
    if (N == 0) return 0;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, c.maxcnt, sh, offsets, theta0, f, gr, &run)) return rc;
    if (int rc = chain_buffers(c, CHAIN_STEPS, MARG_OUT, c.P, "the steps", "steps")) return rc;
    const ChainRecords rec{logp, fullchi2, best};
    auto launch = [&](int t0, int Tc, int kc) {
        launch_two(draws_chain_params_kernel<false>, draws_chain_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, e->stream, ntr, nG, sh.J1, e->jeffreys, Tc,
                   t0, thin, kc, c.kstride, run.rt, e->drw_off, e->drw_theta, e->chn_nacc, run.f, run.W, e->like_mu, e->like_sinv, e->chn_pri, e->chn_step,
                   e->chn_lnu, e->chn_chain, e->chn_rec);
        return 0;
    };
    if (int rc = chain_run(c, step, lnu, chain, &rec, c.K, launch)) return rc;
    if (int rc = chain_fetch(c, last)) return rc;
    return chain_end(c, naccept);
}

int eftb_draws_chain_params(eftb_engine* e, int C, long long N, int T, int thin, const int64_t* offsets, const double* theta0, const double* f,
                            const double* step, const double* lnu, const double* lower, const double* upper, const double* prior_loc,
                            const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept) {
    static const char* who = "eftb_draws_chain_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta0 || !step || !lnu || !chain || !last || !naccept))) return fail("%s: null argument", who);
    return draws_chain_params_impl(e, who, C, N, T, thin, offsets, theta0, f, step, lnu, lower, upper, prior_loc, prior_scale, chain, logp, fullchi2, best,
                                   last, naccept);
}

int eftb_draws_chain_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int T, int thin,
                                     const int64_t* offsets, const double* theta0, const double* f, const double* step, const double* lnu,
                                     const double* lower, const double* upper, const double* prior_loc, const double* prior_scale, double* chain,
                                     double* logp, double* fullchi2, double* best, double* last, int64_t* naccept) {
    static const char* who = "eftb_draws_chain_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || (N > 0 && (!theta0 || !step || !lnu || !chain || !last || !naccept)))
        return fail("%s: null argument", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_chain_params_impl(e, who, G, N, T, thin, offsets, theta0, e->grp_f.data(), step, lnu, lower, upper, prior_loc,
                                   prior_scale, chain, logp, fullchi2, best, last, naccept, &gr);
}

// ------------------------------------------------------------------------------------------------ parallel tempering over the draw parameters
// eftb_draws_temper_params and eftb_draws_temper_params_datasets: the chain call's checks, Gram cache and buffers around
// draws_temper_params_kernel, one workgroup of R waves per ladder.  The swap counts and the sums of ln P persist beside theta and the accept
// counts, and every launch takes its own events out of lnu_swap
static int draws_temper_params_impl(eftb_engine* e, const char* who, int C, long long N, int R, int T, int S, long long first, int thin,
                                    const int64_t* offsets, const double* theta0, const double* f, const double* beta, const double* step, const double* lnu,
                                    const double* lnu_swap, const double* lower, const double* upper, const double* ploc, const double* pscale, double* chain,
                                    double* logp, double* fullchi2, double* best, double* last, int64_t* naccept, int64_t* nswap, double* sum_logp,
                                    const DrawGroups* gr = nullptr) {
    ChainCall c{e, who, N, 0, T, thin};
    if (int rc = chain_front(&c, C, gr ? "group" : "walker", gr ? gr->nwalk : -1, C, 1, offsets, theta0, f, step, lnu, lower, upper, ploc, pscale)) return rc;
    const int ntr = e->ntr, nG = c.nG, P = c.P, npair = std::max(R - 1, 1);
    if (R < 1 || R > TEMPER_MAXR) return fail("%s: R = %d rungs outside [1, %d]", who, R, TEMPER_MAXR);
    for (int w = 0; w < C; ++w)
        if ((offsets[w + 1] - offsets[w]) % R)
            return fail("%s: %s %d owns %lld chains, not a multiple of R = %d rungs", who, gr ? "group" : "walker", w,
                        (long long)(offsets[w + 1] - offsets[w]), R);
    for (int r = 0; r < R; ++r) {
        if (!(beta[r] >= 0.0 && beta[r] <= 1.0)) return fail("%s: beta[%d] = %g outside [0, 1]", who, r, beta[r]);
        if (r && !(beta[r] < beta[r - 1]))
            return fail("%s: beta[%d] = %g is not below beta[%d] = %g: rung %d must be hotter than rung %d", who, r, beta[r], r - 1, beta[r - 1], r, r - 1);
    }
    if (S < 0) return fail("%s: S = %d steps between swap events, at least 0 (no swaps)", who, S);
    if (first < 0) return fail("%s: first_step = %lld, at least 0", who, first);
    const long long nlad = N / R, nsw = S ? (first + T) / S - first / S : 0;  // the ladders of the call and the swap events in it
    if (nsw > 0 && R > 1 && N > 0) {
        if (!lnu_swap) return fail("%s: lnu_swap is NULL with %lld swap events in the call and R = %d rungs", who, nsw, R);
        for (long long l = 0; l < nlad; ++l)
            for (long long j = 0; j < nsw; ++j)
                for (int r = (int)((first / S + j) & 1); r < R - 1; r += 2) {  // (the pairs event j tries: the others are not read)
                    const double v = lnu_swap[(l * nsw + j) * (R - 1) + r];
                    if (!(v <= 0.0))
                        return fail("%s: lnu_swap[%lld][%lld][%d] = %g (ladder, event, rung) is not the logarithm of a uniform in [0, 1]", who, l, j, r, v);
                }
    }
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_CHAIN, &e->recipe[0], &sh)) return rc;
    // a workgroup of R waves and the exchange behind them, whatever the chain call would take
    const size_t xch = TEMPER_XCH * sizeof(double);
    int fit = 0;
    while (fit < TEMPER_MAXR && sh.L.bytes(fit + 1) + xch <= 160 * 1024) ++fit;
    if (R > fit)
        return fail("%s: a ladder of R = %d rungs needs %d waves in one workgroup, but %d fit the LDS beside the Gram matrix of J + 1 = %d columns with "
                    "nG = %d and P = %d parameters", who, R, R, fit, sh.J1, nG, P);
    sh.nw = R;
    sh.lds = sh.L.bytes(R) + xch;
    if (N == 0) return 0;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, c.maxcnt, sh, offsets, theta0, f, gr, &run)) return rc;
    if (int rc = chain_buffers(c, CHAIN_STEPS, MARG_OUT, c.P, "the steps", "steps")) return rc;
    hipStream_t st = e->stream;
    auto events = [&](int t0, int Tc) { return S ? (int)((first + t0 + Tc) / S - (first + t0) / S) : 0; };  // the swap events of the launch at t0
    int most = 0;
    for (int t0 = 0; t0 < T; t0 += CHAIN_STEPS) most = std::max(most, events(t0, std::min(CHAIN_STEPS, T - t0)));
    if (int rc = chain_grow(c, &e->tmp_beta, &e->tmp_beta_cap, TEMPER_MAXR, "beta")) return rc;
    if (int rc = chain_grow(c, &e->tmp_lnus, &e->tmp_lnus_cap, (size_t)nlad * most * (R - 1), "lnu_swap")) return rc;
    if (int rc = chain_grow(c, &e->tmp_sums, &e->tmp_sums_cap, (size_t)N, "the sums of ln P")) return rc;
    if (int rc = chain_grow(c, &e->tmp_nswap, &e->tmp_nswap_cap, (size_t)nlad * npair, "the swap counts", sizeof(long long))) return rc;
    HIPCHK(hipMemcpyAsync(e->tmp_beta, beta, (size_t)R * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(e->tmp_sums, 0, (size_t)N * sizeof(double), st));
    HIPCHK(hipMemsetAsync(e->tmp_nswap, 0, (size_t)nlad * npair * sizeof(long long), st));
    const ChainRecords rec{logp, fullchi2, best};
    auto launch = [&](int t0, int Tc, int kc) {
        // this launch's events of every ladder: step first + t0 is the launch's first, s0 steps remain to its first event, whose global
        // number is g0 / S
        const long long g0 = first + t0;
        const int nswc = events(t0, Tc), s0 = S ? (int)(S - g0 % S) : 0, jpar = S ? (int)((g0 / S) & 1) : 0;
        if (nswc && R > 1) {
            const size_t row = (size_t)nswc * (R - 1) * sizeof(double);
            HIPCHK(hipMemcpy2DAsync(e->tmp_lnus, row, lnu_swap + (size_t)(g0 / S - first / S) * (R - 1), (size_t)nsw * (R - 1) * sizeof(double), row,
                                    (size_t)nlad, hipMemcpyHostToDevice, st));
        }
        launch_two(temper_kernel(false), temper_kernel(true), sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, sh.J1, e->jeffreys, R, Tc, t0, thin, kc,
                   c.kstride, S, s0, jpar, nswc, run.rt, e->drw_off, e->drw_theta, e->chn_nacc, e->tmp_nswap, e->tmp_sums, run.f, run.W, e->like_mu,
                   e->like_sinv, e->chn_pri, e->tmp_beta, e->chn_step, e->chn_lnu, e->tmp_lnus, e->chn_chain, e->chn_rec);
        return 0;
    };
    if (int rc = chain_run(c, step, lnu, chain, &rec, c.K, launch)) return rc;
    e->tmp_host_nswap.resize((size_t)nlad * npair);
    if (int rc = chain_fetch(c, last)) return rc;
    HIPCHK(hipMemcpyAsync(sum_logp, e->tmp_sums, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(e->tmp_host_nswap.data(), e->tmp_nswap, (size_t)nlad * npair * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (int rc = chain_end(c, naccept)) return rc;
    for (long long q = 0; q < nlad * npair; ++q) nswap[q] = e->tmp_host_nswap[q];
    return 0;
}

int eftb_draws_temper_params(eftb_engine* e, int C, long long N, int R, int T, int S, long long first_step, int thin, const int64_t* offsets,
                             const double* theta0, const double* f, const double* beta, const double* step, const double* lnu, const double* lnu_swap,
                             const double* lower, const double* upper, const double* prior_loc, const double* prior_scale, double* chain, double* logp,
                             double* fullchi2, double* best, double* last, int64_t* naccept, int64_t* nswap, double* sum_logp) {
    static const char* who = "eftb_draws_temper_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || !beta || (N > 0 && (!theta0 || !step || !lnu || !chain || !last || !naccept || !nswap || !sum_logp)))
        return fail("%s: null argument", who);
    return draws_temper_params_impl(e, who, C, N, R, T, S, first_step, thin, offsets, theta0, f, beta, step, lnu, lnu_swap, lower, upper, prior_loc,
                                    prior_scale, chain, logp, fullchi2, best, last, naccept, nswap, sum_logp);
}

int eftb_draws_temper_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int R, int T, int S,
                                      long long first_step, int thin, const int64_t* offsets, const double* theta0, const double* f, const double* beta,
                                      const double* step, const double* lnu, const double* lnu_swap, const double* lower, const double* upper,
                                      const double* prior_loc, const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best,
                                      double* last, int64_t* naccept, int64_t* nswap, double* sum_logp) {
    static const char* who = "eftb_draws_temper_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || !beta ||
        (N > 0 && (!theta0 || !step || !lnu || !chain || !last || !naccept || !nswap || !sum_logp)))
        return fail("%s: null argument", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_temper_params_impl(e, who, G, N, R, T, S, first_step, thin, offsets, theta0, e->grp_f.data(), beta, step, lnu, lnu_swap, lower, upper,
                                    prior_loc, prior_scale, chain, logp, fullchi2, best, last, naccept, nswap, sum_logp, &gr);
}

// ------------------------------------------------------------------------------------------------ affine-invariant ensembles over the draw parameters
// eftb_draws_ensemble_params and eftb_draws_ensemble_params_datasets: the chain call's checks (but for its rules on step and lnu), Gram cache
// and buffers around draws_ensemble_params_kernel, one workgroup per ensemble.  z travels where the chain call's step does (one double per
// sweep), lnq where lnu does, and every launch takes its own sweeps out of pick
static int draws_ensemble_params_impl(eftb_engine* e, const char* who, int C, long long N, int K, int T, int thin, const int64_t* offsets,
                                      const double* theta0, const double* f, const double* z, const int32_t* pick, const double* lnq, const double* lower,
                                      const double* upper, const double* ploc, const double* pscale, double* chain, double* logp, double* fullchi2,
                                      double* best, double* last, int64_t* naccept, const DrawGroups* gr = nullptr) {
    ChainCall c{e, who, N, 0, T, thin};
    if (int rc = chain_front(&c, C, gr ? "group" : "walker", gr ? gr->nwalk : -1, C, 1, offsets, theta0, f, nullptr, nullptr, lower, upper, ploc, pscale))
        return rc;
    const int ntr = e->ntr, nG = c.nG, P = c.P;
    if (K < 2 || K > ENS_MAXK || (K & 1)) return fail("%s: K = %d members, not an even number in [2, %d]", who, K, ENS_MAXK);
    for (int w = 0; w < C; ++w)
        if ((offsets[w + 1] - offsets[w]) % K)
            return fail("%s: %s %d owns %lld chains, not a multiple of K = %d members", who, gr ? "group" : "walker", w,
                        (long long)(offsets[w + 1] - offsets[w]), K);
    for (long long q = 0; q < N * T; ++q) {
        const long long n = q / T, t = q % T;
        if (!(z[q] > 0.0) || !std::isfinite(z[q]))
            return fail("%s: z[%lld][%lld] = %g (ensemble %lld, member %lld, sweep %lld) is not a finite stretch factor > 0", who, n, t, z[q], n / K, n % K, t);
        if (pick[q] < 0 || pick[q] >= K / 2)
            return fail("%s: pick[%lld][%lld] = %d (ensemble %lld, member %lld, sweep %lld) outside [0, K / 2 = %d)", who, n, t, (int)pick[q], n / K, n % K, t,
                        K / 2);
        if (!(lnq[q] < INFINITY))
            return fail("%s: lnq[%lld][%lld] = %g (ensemble %lld, member %lld, sweep %lld) is NaN or +inf", who, n, t, lnq[q], n / K, n % K, t);
    }
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_CHAIN, &e->recipe[0], &sh)) return rc;
    // a workgroup of min(ENS_MAXW, K / 2) waves or as many as fit beside the ensemble area, whatever the chain call would take
    sh.nw = sh.L.fit_ens(K, 160 * 1024);
    if (!sh.nw)
        return fail("%s: an ensemble of K = %d members needs %zu bytes of LDS for its states, which leave no room for one wave beside the Gram matrix "
                    "of J + 1 = %d columns with nG = %d and P = %d parameters (%zu bytes per workgroup and %zu per wave, within %d)", who, K,
                    (size_t)K * ENS_SLOT * sizeof(double), sh.J1, nG, P, sh.L.bytes_wg(), sh.L.bytes_wave(), 160 * 1024);
    sh.lds = sh.L.bytes_ens(sh.nw, K);
    if (N == 0) return 0;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, c.maxcnt, sh, offsets, theta0, f, gr, &run)) return rc;
    run.grid = dim3(C, draw_shares(c.maxcnt, K, C));  // (a workgroup takes one ensemble at a time)
    if (int rc = chain_buffers(c, CHAIN_STEPS, MARG_OUT, 1, "the stretch factors", "sweeps")) return rc;
    if (int rc = chain_grow(c, &e->ens_pick, &e->ens_pick_cap, (size_t)N * c.Tmax, "pick", sizeof(int))) return rc;
    hipStream_t st = e->stream;
    const ChainRecords rec{logp, fullchi2, best};
    auto launch = [&](int t0, int Tc, int kc) {
        HIPCHK(hipMemcpy2DAsync(e->ens_pick, (size_t)Tc * sizeof(int), pick + t0, (size_t)T * sizeof(int), (size_t)Tc * sizeof(int), (size_t)N,
                                hipMemcpyHostToDevice, st));
        launch_two(ensemble_kernel(false), ensemble_kernel(true), sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, sh.J1, e->jeffreys, K, Tc, t0, thin, kc,
                   c.kstride, run.rt, e->drw_off, e->drw_theta, e->chn_nacc, run.f, run.W, e->like_mu, e->like_sinv, e->chn_pri, e->chn_step, e->ens_pick,
                   e->chn_lnu, e->chn_chain, e->chn_rec);
        return 0;
    };
    if (int rc = chain_run(c, z, lnq, chain, &rec, c.K, launch)) return rc;
    if (int rc = chain_fetch(c, last)) return rc;
    return chain_end(c, naccept);
}

int eftb_draws_ensemble_params(eftb_engine* e, int C, long long N, int K, int T, int thin, const int64_t* offsets, const double* theta0, const double* f,
                               const double* z, const int32_t* pick, const double* lnq, const double* lower, const double* upper, const double* prior_loc,
                               const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept) {
    static const char* who = "eftb_draws_ensemble_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta0 || !z || !pick || !lnq || !chain || !last || !naccept))) return fail("%s: null argument", who);
    return draws_ensemble_params_impl(e, who, C, N, K, T, thin, offsets, theta0, f, z, pick, lnq, lower, upper, prior_loc, prior_scale, chain, logp, fullchi2,
                                      best, last, naccept);
}

int eftb_draws_ensemble_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int K, int T, int thin,
                                        const int64_t* offsets, const double* theta0, const double* f, const double* z, const int32_t* pick,
                                        const double* lnq, const double* lower, const double* upper, const double* prior_loc, const double* prior_scale,
                                        double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept) {
    static const char* who = "eftb_draws_ensemble_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || (N > 0 && (!theta0 || !z || !pick || !lnq || !chain || !last || !naccept)))
        return fail("%s: null argument", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_ensemble_params_impl(e, who, G, N, K, T, thin, offsets, theta0, e->grp_f.data(), z, pick, lnq, lower, upper, prior_loc, prior_scale, chain,
                                      logp, fullchi2, best, last, naccept, &gr);
}

// ------------------------------------------------------------------------------------------------ Hamiltonian Monte Carlo over the draw parameters
// eftb_draws_hmc_params and eftb_draws_hmc_params_datasets: the chain call's checks (chain_args_check on mom in the place of step), Gram
// cache, prior table and buffers around draws_hmc_params_kernel.  A launch holds at most CHAIN_STEPS gradient evaluations per chain,
// max(1, CHAIN_STEPS / nleap) trajectories; between the launches theta and the accept counts stay on the device and every launch recomputes
// record and gradient of its start, so a chain's bits do not depend on the split
static int draws_hmc_params_impl(eftb_engine* e, const char* who, int C, long long N, int T, int nleap, int thin, const int64_t* offsets, const double* theta0,
                                 const double* f, const double* mom, const double* lnu, const double* eps, const double* factor, const double* lower,
                                 const double* upper, const double* ploc, const double* pscale, double* chain, double* logp, double* fullchi2, double* best,
                                 double* last, int64_t* naccept, double* log_ratio, const DrawGroups* gr = nullptr) {
    ChainCall c{e, who, N, 0, T, thin};
    if (int rc = chain_front(&c, C, gr ? "group" : "walker", gr ? gr->nwalk : -1, C, 1, offsets, theta0, f, mom, lnu, lower, upper, ploc, pscale, "mom"))
        return rc;
    const int ntr = e->ntr, nG = c.nG, P = c.P;
    const eftb_engine::Recipe& rcp = e->recipe[0];
    if (nleap < 1 || nleap > CHAIN_STEPS) return fail("%s: nleap = %d leapfrog steps outside [1, %d]", who, nleap, CHAIN_STEPS);
    for (long long q = 0; q < N * T; ++q)
        if (!(std::isfinite(eps[q]) && eps[q] > 0.0)) return fail("%s: eps[%lld][%lld] = %g is not a finite step size > 0", who, q / T, q % T, eps[q]);
    if (factor)
        for (long long n = 0; n < N; ++n)
            for (int p = 0; p < P; ++p)
                for (int q = 0; q <= p; ++q) {
                    const double v = factor[((size_t)n * P + p) * P + q];
                    if (!std::isfinite(v)) return fail("%s: factor[%lld][%d][%d] is not finite", who, n, p, q);
                    if (q == p && !(v > 0.0)) return fail("%s: factor[%lld][%d][%d] = %g, the diagonal must be > 0", who, n, p, p, v);
                }
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_HMC, &rcp, &sh)) return rc;
    if (!sh.nw)
        return fail("%s: the trajectories of P = %d parameters with nG = %d and J + 1 = %d columns do not fit the LDS (%zu bytes per workgroup and %zu per wave "
                    "of %d)", who, P, nG, sh.J1, sh.L.bytes_wg(), sh.L.bytes_wave(), 160 * 1024);
    if (N == 0) return 0;
    DrawRun run;
    if (int rc = draws_params_begin(e, who, C, N, c.maxcnt, sh, offsets, theta0, f, gr, &run)) return rc;
    if (!e->hmc_lds) {  // the large dynamic LDS for this call's kernel, once per engine (as draws_lds_optin for the others)
        for (const void* k : {reinterpret_cast<const void*>(&draws_hmc_params_kernel<false>), reinterpret_cast<const void*>(&draws_hmc_params_kernel<true>)})
            HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        e->hmc_lds = true;
    }
    if (int rc = chain_buffers(c, std::max(1, CHAIN_STEPS / nleap), MARG_OUT, c.P, "the momenta", "trajectories")) return rc;
    if (int rc = chain_grow(c, &e->hmc_eps, &e->hmc_eps_cap, (size_t)N * c.Tmax, "eps")) return rc;
    if (int rc = chain_grow(c, &e->hmc_ratio, &e->hmc_ratio_cap, (size_t)N * c.Tmax, "the ratios")) return rc;
    if (int rc = chain_grow(c, &e->hmc_fac, &e->hmc_fac_cap, (size_t)N * P * P, "the factors")) return rc;
    RecipeGradTab gt{};
    gt.dcoef = rcp.dcoef;
    gt.pstart = rcp.dtab;
    gt.dent = gt.pstart + P + 1;
    gt.dpack = gt.dent + rcp.ndt;
    gt.erow = gt.dpack + rcp.ndt;
    while ((1 << gt.lgP2) < P) ++gt.lgP2;
    hipStream_t st = e->stream;
    // the lower triangles (NULL: the identity); what lies above the diagonal never reaches the device
    e->hmc_host_fac.assign((size_t)N * P * P, 0.0);
    for (long long n = 0; n < N; ++n)
        for (int p = 0; p < P; ++p)
            for (int q = 0; q <= p; ++q) e->hmc_host_fac[((size_t)n * P + p) * P + q] = factor ? factor[((size_t)n * P + p) * P + q] : (q == p ? 1.0 : 0.0);
    HIPCHK(hipMemcpyAsync(e->hmc_fac, e->hmc_host_fac.data(), (size_t)N * P * P * sizeof(double), hipMemcpyHostToDevice, st));
    e->hmc_host_ratio.resize((size_t)N * c.Tmax);
    const ChainRecords rec{logp, fullchi2, best};
    auto launch = [&](int t0, int Tc, int kc) {
        HIPCHK(hipMemcpy2DAsync(e->hmc_eps, (size_t)Tc * sizeof(double), eps + t0, (size_t)T * sizeof(double), (size_t)Tc * sizeof(double), (size_t)N,
                                hipMemcpyHostToDevice, st));
        launch_two(draws_hmc_params_kernel<false>, draws_hmc_params_kernel<true>, sh.J1, run.grid, run.block, sh.lds, st, ntr, nG, sh.J1, e->jeffreys, Tc, t0, thin, kc,
                   c.kstride, nleap, run.rt, gt, e->drw_off, e->drw_theta, e->chn_nacc, run.f, run.W, e->like_mu, e->like_sinv, e->chn_pri, e->chn_step, e->chn_lnu,
                   e->hmc_eps, e->hmc_fac, e->chn_chain, e->chn_rec, e->hmc_ratio);
        return 0;
    };
    ChainMore ratios;  // with log_ratio every launch is waited for: the ratios of one that stores no state come back too
    if (log_ratio)
        ratios = [&](int t0, int Tc, bool landed) {
            if (!landed) {
                HIPCHK(hipMemcpyAsync(e->hmc_host_ratio.data(), e->hmc_ratio, (size_t)N * Tc * sizeof(double), hipMemcpyDeviceToHost, st));
                return 0;
            }
            for (long long n = 0; n < N; ++n) std::copy_n(e->hmc_host_ratio.data() + (size_t)n * Tc, Tc, log_ratio + (size_t)n * T + t0);
            return 0;
        };
    if (int rc = chain_run(c, mom, lnu, chain, &rec, c.K, launch, ratios)) return rc;
    if (int rc = chain_fetch(c, last)) return rc;
    return chain_end(c, naccept);
}

int eftb_draws_hmc_params(eftb_engine* e, int C, long long N, int T, int nleap, int thin, const int64_t* offsets, const double* theta0, const double* f,
                          const double* mom, const double* lnu, const double* eps, const double* factor, const double* lower, const double* upper,
                          const double* prior_loc, const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last,
                          int64_t* naccept, double* log_ratio) {
    static const char* who = "eftb_draws_hmc_params";
    if (e) sub_drain(e);
    if (!e || !offsets || !f || (N > 0 && (!theta0 || !mom || !lnu || !eps || !chain || !last || !naccept))) return fail("%s: null argument", who);
    return draws_hmc_params_impl(e, who, C, N, T, nleap, thin, offsets, theta0, f, mom, lnu, eps, factor, lower, upper, prior_loc, prior_scale, chain, logp,
                                 fullchi2, best, last, naccept, log_ratio);
}

int eftb_draws_hmc_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int T, int nleap, int thin,
                                   const int64_t* offsets, const double* theta0, const double* f, const double* mom, const double* lnu, const double* eps,
                                   const double* factor, const double* lower, const double* upper, const double* prior_loc, const double* prior_scale,
                                   double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept, double* log_ratio) {
    static const char* who = "eftb_draws_hmc_params_datasets";
    if (e) sub_drain(e);
    if (!e || !walker || !dataset || !offsets || !f || (N > 0 && (!theta0 || !mom || !lnu || !eps || !chain || !last || !naccept)))
        return fail("%s: null argument", who);
    DrawGroups gr{0, walker, dataset};
    if (int rc = draws_groups_check(e, who, C, G, f, &gr)) return rc;
    return draws_hmc_params_impl(e, who, G, N, T, nleap, thin, offsets, theta0, e->grp_f.data(), mom, lnu, eps, factor, lower, upper, prior_loc, prior_scale,
                                 chain, logp, fullchi2, best, last, naccept, log_ratio, &gr);
}

// ------------------------------------------------------------------------------------------------ dragging chains between two walkers
// eftb_draws_drag_params: the chain call's checks (chain_args_check, thin = 0 allowed), Gram cache (W_c of the C walkers), prior table,
// buffers and split into launches of CHAIN_STEPS steps around draws_drag_params_kernel.  C walkers are resident; pair g = (wstart[g], wend[g])
// owns the chains offsets[g] ... offsets[g + 1] - 1.  Between the launches theta, the accept counts and the sums [N][2] stay on the device;
// every launch recomputes both records of its starting theta, so a chain's bits do not depend on the split.  The record arrays have
// K + 1 slots per chain: the K stored records, then the one of the state after step T
int eftb_draws_drag_params(eftb_engine* e, int C, int G, const int32_t* wstart, const int32_t* wend, long long N, int T, int thin, const int64_t* offsets,
                           const double* theta0, const double* f, const double* frac, const double* step, const double* lnu, const double* lower,
                           const double* upper, const double* prior_loc, const double* prior_scale, double* chain, double* logp_start, double* logp_end,
                           double* fullchi2_start, double* fullchi2_end, double* best_start, double* best_end, double* last, int64_t* naccept, double* sums) {
    static const char* who = "eftb_draws_drag_params";
    if (e) sub_drain(e);
    if (!e || !wstart || !wend || !offsets || !f || !frac || (N > 0 && (!theta0 || !step || !lnu || !last || !naccept || !sums)))
        return fail("%s: null argument", who);
    if (C < 1) return fail("%s: %d walkers", who, C);
    ChainCall c{e, who, N, 0, T, thin};
    if (int rc = chain_front(&c, G, "pair", C, C, 0, offsets, theta0, f, step, lnu, lower, upper, prior_loc, prior_scale)) return rc;
    const int ntr = e->ntr, nG = c.nG, P = c.P;
    if (thin > 0 && N > 0 && !chain) return fail("%s: null argument (chain, with thin = %d)", who, thin);
    for (int g = 0; g < G; ++g) {
        if (wstart[g] < 0 || wstart[g] >= C) return fail("%s: wstart[%d] = %d outside [0, %d): the start walker of pair %d", who, g, wstart[g], C, g);
        if (wend[g] < 0 || wend[g] >= C) return fail("%s: wend[%d] = %d outside [0, %d): the end walker of pair %d", who, g, wend[g], C, g);
    }
    for (int t = 0; t < T; ++t)
        if (!(frac[t] >= 0.0 && frac[t] <= 1.0)) return fail("%s: frac[%d] = %g outside [0, 1]", who, t, frac[t]);
    DrawShape sh;
    if (int rc = draws_logp_shape(e, who, DRAW_DRAG, &e->recipe[0], &sh)) return rc;
    if (!sh.nw)
        return fail("%s: the call stages two Gram matrices of J + 1 = %d columns per workgroup; with nG = %d they do not fit the LDS beside one wave (%zu bytes per "
                    "workgroup and %zu per wave of %d)", who, sh.J1, nG, sh.L.bytes_wg(), sh.L.bytes_wave(), 160 * 1024);
    if (N == 0) return 0;
    constexpr int PAIR = 2 * MARG_OUT;
    if (int rc = draws_logp_begin(e, who, G, N, sh.J1, offsets, C)) return rc;
    if (!e->drg_lds) {  // the large dynamic LDS for this call's kernel, once per engine (as draws_lds_optin for the others)
        for (const void* k : {reinterpret_cast<const void*>(&draws_drag_params_kernel<false>), reinterpret_cast<const void*>(&draws_drag_params_kernel<true>)})
            HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        e->drg_lds = true;
    }
    const double *dtheta = nullptr, *df = nullptr;
    if (int rc = draws_params_upload(e, P, C, N, theta0, f, &dtheta, &df)) return rc;
    const dim3 grid(G, draw_shares(c.maxcnt, sh.nw, G)), block(64 * sh.nw);
    const RecipeTab rt = recipe_tab(e->recipe[0]);
    if (int rc = chain_buffers(c, CHAIN_STEPS, PAIR, c.P, "the steps", "steps")) return rc;
    if (int rc = chain_grow(c, &e->drg_pair, &e->drg_pair_cap, 2 * (size_t)G, "the pairs", sizeof(int))) return rc;
    if (int rc = chain_grow(c, &e->drg_frac, &e->drg_frac_cap, (size_t)T, "frac")) return rc;
    if (int rc = chain_grow(c, &e->drg_sums, &e->drg_sums_cap, 2 * (size_t)N, "the sums")) return rc;
    if (int rc = chain_grow(c, &e->drg_fin, &e->drg_fin_cap, (size_t)N * PAIR, "the final records")) return rc;
    hipStream_t st = e->stream;
    e->drg_host_pair.assign(wstart, wstart + G);
    e->drg_host_pair.insert(e->drg_host_pair.end(), wend, wend + G);
    HIPCHK(hipMemcpyAsync(e->drg_pair, e->drg_host_pair.data(), 2 * (size_t)G * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->drg_frac, frac, (size_t)T * sizeof(double), hipMemcpyHostToDevice, st));
    const ChainRecords rec[2] = {{logp_start, fullchi2_start, best_start}, {logp_end, fullchi2_end, best_end}};
    auto launch = [&](int t0, int Tc, int kc) {
        launch_two(draws_drag_params_kernel<false>, draws_drag_params_kernel<true>, sh.J1, grid, block, sh.lds, st, ntr, nG, sh.J1, e->jeffreys, Tc, t0, thin, kc,
                   c.kstride, rt, e->drw_off, e->drg_pair, e->drg_pair + G, e->drw_theta, e->chn_nacc, e->drg_sums, df, e->drw_W, e->like_mu, e->like_sinv, e->chn_pri,
                   e->drg_frac, e->chn_step, e->chn_lnu, e->chn_chain, e->chn_rec, e->drg_fin);
        return 0;
    };
    if (int rc = chain_run(c, step, lnu, chain, rec, c.K + 1, launch)) return rc;
    e->drg_host_fin.resize((size_t)N * PAIR);
    if (int rc = chain_fetch(c, last)) return rc;
    HIPCHK(hipMemcpyAsync(sums, e->drg_sums, 2 * (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(e->drg_host_fin.data(), e->drg_fin, (size_t)N * PAIR * sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = chain_end(c, naccept)) return rc;
    for (long long n = 0; n < N; ++n)  // the records of the state after step T: the last slot
        for (int r = 0; r < 2; ++r)
            draws_unpack(e->drg_host_fin.data() + (size_t)n * PAIR + r * MARG_OUT, nG, (size_t)n * (c.K + 1) + c.K, rec[r].logp, rec[r].fullchi2, rec[r].best);
    return 0;
}

// (the one place that names draws_temper_params_kernel: see the declaration above draws_lds_optin)
static TemperKernel temper_kernel(bool two) { return two ? &draws_temper_params_kernel<true> : &draws_temper_params_kernel<false>; }
// (and the one place that names draws_ensemble_params_kernel)
static EnsembleKernel ensemble_kernel(bool two) { return two ? &draws_ensemble_params_kernel<true> : &draws_ensemble_params_kernel<false>; }
