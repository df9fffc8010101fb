/*
 * eftbird.h -- C ABI of the MI355X-native EFTofLSS one-loop engine (libeftbird.so).
 *
 * Drop-in boundary for the PyBird theory-vector hot path of zhaoruiyang98/eftpipe.  The reference has
 * no FFI (it is pure Python); each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  The host side (the eftpipe_amd Python package) binds these with ctypes and
 * re-exposes the reference's own class surface (Common, Bird, NonLinear.PsCf, Bird.setPsCfl, Resum.Ps,
 * APeffect.AP, Window.Window, Binning.transform, Chained.transform, reduce_Plk).
 *
 * Conventions: plain C types only; all arrays are C-contiguous float64 unless stated; the caller owns
 * every host buffer, the library owns the engine and all device memory; one engine per (process, GPU),
 * not re-entrant per engine.  Every function returns 0 on success, non-zero on error; the message is
 * available from eftb_last_error().  There is NO CPU fallback: without a HIP device eftb_create fails.
 */
#ifndef EFTBIRD_H
#define EFTBIRD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eftb_engine eftb_engine;

/* Dimensions + switches fixed at construction.  Replaces the constructor arguments of
 * pybird.Common (eftpipe/pybird/pybird.py:498-514), pybird.NonLinear (:907-915), pybird.Resum (:1230),
 * pybird.APeffect (:1503-1518) as used by EFTLeafKernel.initialize_with_provider (eftpipe/theory.py:423-495). */
typedef struct eftb_config {
    int32_t device;        /* HIP device ordinal */
    int32_t Nl;            /* multipoles computed: 2 (l=0,2) or 3 (l=0,2,4)            Common.Nl */
    int32_t Nk;            /* |co.k|                                                    Common.Nk */
    int32_t Nkin;          /* |kin| of the input linear spectrum (200)                  theory.py:562 */
    int32_t max_batch;     /* device state is sized for this many cosmologies per call */
    int32_t with_resum;    /* IR-resummation on (needs the C11/Cct/C22/C13 pieces)      theory.py:573 */
    int32_t with_ap;       /* Alcock-Paczynski on                                       theory.py:582 */
    int32_t ap_stochastic; /* APeffect(APst=True): distort Pstl too                     pybird.py:1618 */
    int32_t nmu;           /* AP mu nodes (nbinsmu*accboost)                            pybird.py:1538 */
    int32_t ntail;         /* power-law tail length of the loop FFTLog (high-k columns, then the ntail_lo low-k ones)   fftlog.py:140-151 */
    int32_t nxtail;        /* same for the 32-point IR-filter FFTLog (then the nxtail_lo low-k ones)                   pybird.py:1293 */
    int32_t nbasis;        /* dimension of the span of the 28 M22 loop matrices (7)     tables.py loop_basis */
    int32_t nbasis13;      /* dimension of the span of the 10 M13 vectors (2)           tables.py loop_basis */
    int32_t NIR, Na, Nklow;/* Resum.NIR, Resum.Na, Common.Nklow                         pybird.py:1247-1259, 560 */
    int32_t with_nnlo;     /* Common.with_NNLO: the k^4 P11 counter-terms PctNNLOl       pybird.py:741-748, 1447-1458, 1615 */
    int32_t optiresum;     /* Common.optiresum: only the BAO peak is resummed (EFTB_T_BAO); the s axis keeps 80 slots, the first 52
                              hold arange(70, 200, 2.5), the rest repeat the last value and carry no weight   pybird.py:553-556, 1382-1400 */
    int32_t dual_coef;     /* Common.IRcutoff = "loop" | "resum": the xi-space pieces use a second FFTLog operator (EFTB_T_GCT2)
                              pybird.py:1151-1160  ("all" needs no switch: both operators are the cut one) */
    int32_t step_batch;    /* largest batch of ONE staged step (0 = max_batch).  With step_batch < max_batch, staged steps that are still queued
                              when the submission thread reaches them are launched TOGETHER, as one batch of up to max_batch cosmologies (same
                              bits per cosmology; each step is still fetched by itself).  No reference counterpart. */
    /* appended fields (0 = the behaviour before they existed) */
    int32_t nfft;          /* loop FFTLog size NonLinear(NFFT): even, 256..512; 0 = 256.  NCH = nfft / 2 + 1 independent coefficients,
                              NPOW = nfft + 1 powers                                    pybird.py:907-919 */
    int32_t ntail_lo;      /* input grids starting above the FFTLog's xmin = 1.5e-5: the last ntail_lo of the ntail tail columns continue Pin
                              below kin[0] (slope and amplitude of its first two samples, which must then be positive)   fftlog.py:140-145 */
    int32_t nxtail_lo;     /* same for the IR-filter FFTLog: the last nxtail_lo of the nxtail columns; EFTB_T_WQLAST2 then holds 4 weights */
} eftb_config;

/* Constant tables (built on the host by eftpipe_amd/tables.py; shapes in that file).  The first-stage operators are stored as GEMM operands,
 * K-major and zero padded to KP(n) = n rounded up to a multiple of 48 (the K chunk of the matrix-core kernel):
 *   EFTB_T_SKT [KP(Nkin)][Nk]                   P11 = Pin . SKT                                        (pybird.py:694-695)
 * Sizes that follow the loop FFTLog are written with NCH = nfft / 2 + 1 (129 at the default 256), NPOW = 2 NCH - 1 and NH = NCH - 1:
 *   EFTB_T_GCT [KP(Nkin + ntail)][2 * NCH]      FFTLog coefficients (re | im halves) = [Pin | tail] . GCT   (fftlog.py:84-166)
 *   EFTB_T_ECT [2 * NCH][KP(Nkin + ntail)]      = GCT transposed: the same product with the batch as the column dimension
 *   EFTB_T_BXT [KP(Nkin + nxtail)][2 * 80]      IR filters X | Y = [Pin | tail'] . BXT                 (pybird.py:1316-1353)
 *   EFTB_T_GCT2, EFTB_T_GCT2T                   the layouts of GCT, ECT
 *   EFTB_T_AD [NPOW][NH + 2][nbasis (+ nbasis13)] complex    anti-diagonal pair weights (tables.antidiagonal_tables)
 *   EFTB_T_MLJ [Nl][NPOW] complex, EFTB_T_LINVEC [10 (+ 2|3 Nl)][NCH] complex
 *   EFTB_T_SYNK / SYNS [KP(4 NH + 1)][Nk | 80], EFTB_T_LINK / LINS [KP(2 NH + 1)][Nk | 80]   synthesis bases (tables.synthesis_table)
 *   EFTB_T_WQLAST2 [2] exp(-k^2/L^2)/k^2 at the last two kin (+ at the first two when nxtail_lo > 0)
 *   EFTB_T_SPCBAND [65][Nk], EFTB_T_SPLOCAL [Nk][4][4]   the AP splines in B-spline form: coefficient operator and per-interval pieces (tables.bspline_tables)
 * (EFTB_T_TYT is an unused id kept for numbering.) */
enum eftb_table {
    EFTB_T_K = 0, EFTB_T_S, EFTB_T_LNKIN, EFTB_T_SKT, EFTB_T_GCT, EFTB_T_ECT, EFTB_T_LNXTAIL,
    /* one-loop pieces in anti-diagonal form (tables.py antidiagonal_tables, synthesis_table) */
    EFTB_T_AD, EFTB_T_EXP22, EFTB_T_EXPC, EFTB_T_MLJ, EFTB_T_LINVEC, EFTB_T_SYNK, EFTB_T_SYNS, EFTB_T_LINK, EFTB_T_LINS,
    EFTB_T_L11, EFTB_T_LCT, EFTB_T_L22, EFTB_T_L13, EFTB_T_GRP,
    EFTB_T_BXT, EFTB_T_SPCBAND, EFTB_T_SPLOCAL, EFTB_T_TYT, EFTB_T_LNXXTAIL, EFTB_T_WQLAST2, EFTB_T_QPOLY, EFTB_T_H,
    EFTB_T_RSBASIS, EFTB_T_RSBASISS, EFTB_T_RSROWS,   /* matrix-core IR-resummation (Nl = 3): tables.py resum_mfma_tables */
    EFTB_T_MU, EFTB_T_WMU, EFTB_T_LEGMU, EFTB_T_SPBAND, EFTB_T_APFID,
    EFTB_T_LCTN,      /* with_nnlo: Common.lctNNLO [Nl][3] zero padded to [Nl][6]     pybird.py:575 */
    EFTB_T_BAO,       /* optiresum: a(s)[80], b(s)[80], then i_lo, i_hi, i_first, i_end as doubles: inside [i_first, i_end)
                         bao(s) = C(s) - a(s) C(s[i_lo]) - b(s) C(s[i_hi]), 0 elsewhere     Resum.extractBAO pybird.py:1382-1400 */
    EFTB_T_GCT2,      /* dual_coef: FFTLog operator of the xi-space coefficients (layout of EFTB_T_GCT) */
    EFTB_T_GCT2T,     /* dual_coef: its transpose (layout of EFTB_T_ECT) */
    EFTB_T_QEPOLY,    /* Nl = 3: [2][Nl Nl 2 8 Na][15] Q(f) of direct-P_l runs in the closed-form basis (tables.py resum_plk_tables; layout of EFTB_T_QPOLY) */
    EFTB_T_COUNT
};


/* Device-resident state (per engine, [max_batch] leading axis unless noted). */
enum eftb_buffer {
    EFTB_B_PIN = 0,   /* [B][Nkin]            Bird.Pin                            pybird.py:693 */
    EFTB_B_F,         /* [B]                  Bird.f                                              */
    EFTB_B_DA,        /* [B]                  Bird.DA                                             */
    EFTB_B_H,         /* [B]                  Bird.H                                              */
    EFTB_B_P11,       /* [B][Nk]              Bird.P11                            pybird.py:695 */
    EFTB_B_P22,       /* [B][28][Nk]          Bird.P22                            pybird.py:1076 */
    EFTB_B_P13,       /* [B][10][Nk]          Bird.P13                            pybird.py:1082 */
    EFTB_B_C11,       /* [B][Nl][80]          Bird.C11                            pybird.py:1090 */
    EFTB_B_CCT,       /* [B][Nl][80]          Bird.Cct                            pybird.py:1094 */
    EFTB_B_CC,        /* [B][Nl*38][80]       Bird.C22 ([Nl][28][80]) then Bird.C13 ([Nl][10][80]) */
    EFTB_B_CLOOPL,    /* [B][Nl][12][80]      Bird.Cloopl                         pybird.py:805-846   (written by a REGROUP stage that is not
                                              followed by RESUM in the same run: whole-pipeline runs regroup straight into the resummation records) */
    EFTB_B_TEMPL,     /* [B][nl][24][nx]      rows 0-2 P11l, 3-8 Pctl, 9-20 Ploopl, 21-23 Pstl; (nl, nx) = (Nl, Nk) until an
                                              operator (window / binning / chained) is applied, then that operator's output shape */
    EFTB_B_XY,        /* [B][2][80]           IR filters X(s), Y(s)               pybird.py:1316-1353 */
    EFTB_B_Q,         /* [B][2][Nl][Nl][Nn]   Resum.Q                             pybird.py:1367-1380 */
    EFTB_B_BIAS,      /* [B][24]              b11(3), bct(6), bloop(12), bst(3)   parambasis.py:69-126 */
    EFTB_B_PLK,       /* [B][nl][nx]          reduce_Plk(...).sum() without Picc  parambasis.py:128-136 */
    EFTB_B_COEF,      /* [B][2][NCH]          FFTLog coefficients (independent half, re/im) */
    EFTB_B_GROWS,     /* [B][25][24]          coefficient rows of P_NG (row 0) and dP/d(gaussian parameter) (rows 1..nG)   parambasis.py:249-316 */
    EFTB_B_LOGP,      /* [B][26]              marginalised ln P, full chi2 at the best fit, best-fit gaussian parameters  marginal.py:79-140 */
    /* with_nnlo only.  The NNLO counter-terms travel as a second template block whose Pctl slots (rows 3-5) hold PctNNLOl and
     * whose other rows are zero: every linear stage (Resum with Q[1] and lctNNLO, AP, the operators) runs on it unchanged. */
    EFTB_B_CCTN,      /* [B][Nl][80]          Bird.CctNNLO                        pybird.py:1098-1101 */
    EFTB_B_TEMPLN,    /* [B][nl][24][nx]      rows 3-5 = Bird.PctNNLOl            pybird.py:741-748 */
    EFTB_B_BIASN,     /* [B][3]               bctNNLO                             parambasis.py:96-106 */
    EFTB_B_GROWSN,    /* [B][25][3]           NNLO part of the EFTB_B_GROWS rows: coefficients of PctNNLOl in P_NG (row 0) and in
                                              dP/d(cr4, cr6 | ctilde) (parambasis.py:303-307, 429-435); zero-initialised */
    EFTB_B_COUNT
};

/* Stages, in the order EFTLeafKernel.calculate_power_spectrum runs them (theory.py:557-609). */
enum eftb_stage {
    EFTB_S_PREP    = 1 << 0,  /* Bird.__init__ spline + NonLinear.Coef        pybird.py:694-695, 1127-1141 */
    EFTB_S_LOOPS   = 1 << 1,  /* makeP22, makeP13                             pybird.py:1074-1086 */
    EFTB_S_CF      = 1 << 2,  /* makeC11, makeCct, makeC22, makeC13           pybird.py:1088-1125 */
    EFTB_S_REGROUP = 1 << 3,  /* Bird.setPsCfl                                pybird.py:737-866 */
    EFTB_S_RESUM   = 1 << 4,  /* Resum.Ps                                     pybird.py:1413-1464 */
    EFTB_S_AP      = 1 << 5,  /* APeffect.AP                                  pybird.py:1598-1621 */
    EFTB_S_PROJECT = 1 << 6,  /* the pipeline operator (eftb_set_pipeline_operator): Window.Window / Binning / Chained, folded
                                 window.py:371-415, binning.py:131-162, chained.py:56-68 */
    EFTB_S_REDUCE  = 1 << 7,  /* reduce_Plk                                   parambasis.py:42-136 */
    EFTB_S_ALL     = 0xff,
    /* single-kernel selectors (profiling / roofline measurement only; need the stage's inputs in place) */
    EFTB_K_P22     = 1 << 8,  /* makeP22 alone: anti-diagonal sums + rows + synthesis */
    EFTB_K_C22     = 1 << 9,  /* makeC22 + makeC13 alone */
    EFTB_K_RESUM   = 1 << 10, /* the main kernel of Resum.Ps alone (operands of an earlier EFTB_S_RESUM run) */
    EFTB_S_LOGP    = 1 << 11, /* Marginalizable.marginalized_logp on the current template block   marginal.py:79-140 */
    EFTB_K_IRFILTER = 1 << 12 /* Resum.IRFilters + Resum.makeQ alone: X(s), Y(s), Q(f) from the inputs (EFTB_B_XY, EFTB_B_Q)   pybird.py:1316-1380 */
};

int  eftb_create(const eftb_config* cfg, eftb_engine** out);
int  eftb_set_table(eftb_engine* e, int table_id, const void* host, size_t nbytes);
int  eftb_finalize(eftb_engine* e);
void eftb_destroy(eftb_engine* e);

/* Run-time switches that the reference keeps on plugin objects rather than on Common. */
enum eftb_option {
    EFTB_O_AP_STOCHASTIC = 0, /* APeffect.APst                                pybird.py:1514, 1618 */
    EFTB_O_JEFFREYS = 1,      /* marginalized_logp(jeffreys=True): drop ln det(F2 / 2 pi)   marginal.py:118-121 */
    EFTB_O_GRAPH = 2,         /* replay whole-pipeline runs (stage masks starting at PREP) from captured HIP graphs: one host call per
                                 step; for busy hosts (no reference counterpart; off by default, also EFTB_GRAPH=1) */
    EFTB_O_CHECK_FINITE = 3,  /* the REDUCE stage flags non-finite P_l(k): the next synchronising call (eftb_sync, eftb_get, eftb_eval_*,
                                 eftb_fetch_*) then returns non-zero naming the cosmology (off by default) */
    EFTB_O_TIME_DOMINANT = 4  /* value n > 0: bracket every n-th launch of the resummation kernel with HIP events on the stream it runs on
                                 (measurement only: bench.py's roofline; read with eftb_dominant_time; inactive while EFTB_O_GRAPH replays
                                 captured runs).  The two event packets cost the pipelined loop about 1.5 % when every launch carries them. */,
    EFTB_O_LATENCY_MODE = 5,  /* 1 (default): a step staged (eftb_stage_inputs) while the GPU is idle runs in latency mode -- one queue, P_lin read from
                                 the staging block, P_l written to mapped host memory by the kernel that forms it: what a sampler wants whose next
                                 step depends on this step's result.  0: always the three-stream layout (a caller that knows more steps follow
                                 at once: the first step of a pipelined loop then does not hold the main queue with its AP stage) */
    EFTB_O_PLK_DIRECT = 6,    /* 1: whole-pipeline runs that end in REDUCE (PREP .. AP | REDUCE, no PROJECT / LOGP; Nl = 3, fast AP path) take the
                                 bias contraction of reduce_Plk (parambasis.py:42-136) FIRST -- it commutes with Resum.Ps and APeffect.AP, linear maps
                                 that act on every template row alike (pybird.py:1413-1464, 1581-1621) -- so one row per multipole instead of 24
                                 goes through them: same P_l(k) (summation order aside), but EFTB_B_TEMPL does not hold the templates of such a
                                 run, and the stage taps EFTB_B_P13 / C11 / CCT (and the synthesised basis rows behind P22 / CC) hold rows already
                                 CONTRACTED with the bias.  Only a run whose mask holds PREP, LOOPS, CF, REGROUP, RESUM, AP and REDUCE together is
                                 taken this way: a sequence split into several eftb_run calls always takes the template path.
                                 0 (default): templates first, as the reference computes them (BirdSnapshot semantics) */
    EFTB_O_TIME_KERNEL = 7,   /* which launches EFTB_O_TIME_DOMINANT brackets, a set of: 1 (default) the resummation kernel, 2 the synthesis launch of
                                 the loop stages (synth_kernel), 4 the heaviest AP kernel (ap_weights_kernel; direct-P_l runs: ap_plk_kernel) -- measurement only */
    EFTB_O_STEP_TRACE = 10,   /* measurement: timing events at nine points of every staged direct-P_l launch (upload start, front end, synthesis start,
                                 operand build end, resummation start / end, spline start, AP end, copy-out end), each on its own stream; read with
                                 eftb_step_trace.  Switching it on (again) restarts the clock. */
    EFTB_O_SUBMIT_HOLD = 9,   /* tests: 1 makes the submission thread leave queued steps where they are until the option is cleared (or any entry point
                                 that needs the queue empty is called) -- the steps queued meanwhile then leave together, as eftb_config.step_batch allows */
    EFTB_O_SUBMIT_THREAD = 8  /* 1 (default; also EFTB_SUBMIT_THREAD=0/1): staged steps handed in while earlier ones are still queued or running are
                                 issued by a submission thread inside the library -- eftb_stage_inputs fills the page-locked block, eftb_run_staged
                                 queues the step and returns; the thread uploads the block and launches the kernels (50-95 us of HIP calls per step
                                 that the sampler's thread no longer pays).  A step staged while the engine is quiescent and the GPU idle is issued by
                                 the caller as before.  Same bits either way.  0: the caller's thread issues every step; 2: every step is queued, whatever the
                                 GPU is doing (tests).  No reference counterpart. */
};
int  eftb_set_option(eftb_engine* e, int option, int value);
/* Sum of the event-bracketed durations [ms] and number of resummation launches since the last reset (EFTB_O_TIME_DOMINANT); waits for
 * the launches still in flight. */
int  eftb_dominant_time(eftb_engine* e, double* ms_sum, long long* launches, int reset);
/* The same for one of the launches EFTB_O_TIME_KERNEL selects: kind 0 the resummation kernel (= eftb_dominant_time), 1 the synthesis launch, 2 the AP
 * kernel. */
int  eftb_kernel_time(eftb_engine* e, int kind, double* ms_sum, long long* launches, int reset);
/* ... and the cosmologies those launches carried: a launch of coalesced staged steps (eftb_config.step_batch) carries several steps' batches. */
int  eftb_kernel_time_ex(eftb_engine* e, int kind, double* ms_sum, long long* launches, long long* cosmologies, int reset);

/* Likelihood of the EFTB_S_LOGP stage.  Replaces, for a batch of walkers on the device,
 * EFTLike.PNG / PG (likelihood.py:483-549: flatten the multipoles over the masked k bins) and
 * Marginalizable.marginalized_logp (marginal.py:79-140).  index[a] = l * nx + x selects data point a from the current
 * template block [nl][24][nx] (after the pipeline operator, if any); data[ndata]; invcov[ndata][ndata] symmetric;
 * 0 <= nG <= 24 marginalised parameters (nG = 0: the plain Gaussian likelihood -chi2 / 2 of row 0) with Gaussian prior N(mu[i], sigma_i^2), sigma_inv[i] = 1 / sigma_i^2 (all zero: flat).
 * Per walker the caller puts the coefficient rows EFTB_B_GROWS (eftpipe_amd.parambasis.gaussian_rows) and reads
 * EFTB_B_LOGP after eftb_run(..., EFTB_S_LOGP, B). */
int  eftb_set_likelihood(eftb_engine* e, int ndata, const int32_t* index, const double* data, const double* invcov,
                         int nG, const double* mu, const double* sigma_inv);

/* Linear post-AP projections.  Window.Window (window.py:371-415), Binning.transform (binning.py:131-162) and
 * Chained.transform (chained.py:56-68) are linear maps of the template block on the k axis and the multipole
 * axis; each is registered once as a dense operator  out[a][row][x] = sum_{l,k} op[a][l][x][k] * in[l][row][k]
 * (the cubic splines onto the window p grid / the bin quadrature points are folded in on the host) and applied
 * on the FP64 matrix cores.  `op` is [nl_out][nl_in][nx_out][nx_in]; requires nl_out*nx_out <= Nl*Nk. */
int  eftb_add_operator(eftb_engine* e, int nl_out, int nx_out, int nl_in, int nx_in, const double* op, int* op_id);
/* The stochastic rows (Pstl, rows 21-23) of operator `op_id` go through the matrix of `st_op_id` (same shape) instead:
 * Window(window_st=False) (window.py:412-415) and FiberCollision(fiberst=False) (pybird.py:1788-1797) leave Pstl alone while
 * binning / chained still act on it.  st_op_id = -1 restores one matrix for all rows. */
int  eftb_set_operator_stochastic(eftb_engine* e, int op_id, int st_op_id);
/* Several tracers per likelihood point (EFTLike(tracers=[LRG, ELG, X]): reference likelihood.py:483-549, cfg 3 of BASELINE).
 * The batch then holds ntr consecutive entries per walker (entry = walker * ntr + tracer), each with its own P_lin, f, DA, H
 * (for a per-tracer AP fiducial pass DA * DA_fid_engine / DA_fid_tracer and H * H_fid_engine / H_fid_tracer) and bias rows.
 *  - eftb_set_pipeline_operator_tracer: the PROJECT stage uses operator op_id for the entries of `tracer` (window / fibre /
 *    binning / chained differ per tracer); all operators must share one shape -- pad a chained output with zero multipoles;
 *  - the LOGP stage treats the ntr entries of a walker as ONE block of ntr * nl multipoles: index[a] = (tracer * nl + l) * nx + x,
 *    rows (EFTB_B_GROWS) per entry with zero rows for the parameters that do not act on that tracer, results per walker
 *    (EFTB_B_LOGP [B / ntr][26], eftb_eval_logp_batch outputs [B / ntr]).
 * eftb_set_tracers resets the per-tracer operators and the likelihood; call it first. */
int  eftb_set_tracers(eftb_engine* e, int ntr);
int  eftb_set_pipeline_operator_tracer(eftb_engine* e, int tracer, int op_id);
/* Apply to the current template block of cosmologies [0, B); the block takes the operator's output shape. */
int  eftb_apply_operator(eftb_engine* e, int op_id, int B);
/* Operator run by the EFTB_S_PROJECT stage of eftb_run / eftb_eval_batch (-1 = none). */
int  eftb_set_pipeline_operator(eftb_engine* e, int op_id);
/* Declare the shape of the template block before eftb_put(EFTB_B_TEMPL, ...) of already-projected templates. */
int  eftb_set_template_dims(eftb_engine* e, int nl, int nx);

/* Input guards.  P_lin must be finite, and positive at its last two samples: the FFTLog extrapolates it beyond kin[-1] with the power
 * law through them (reference fftlog.py:146-151 takes their logarithm), and, when the grid starts above the FFTLog's xmin (ntail_lo or
 * nxtail_lo > 0), at its first two samples as well (fftlog.py:140-145); f must be finite, DA and H finite and positive.  The entry
 * points that take host inputs (eftb_eval_batch, eftb_eval_logp_batch, eftb_stage_inputs) check this before anything is copied and
 * return non-zero; for inputs placed with eftb_put the first kernel raises a flag instead and the next synchronising call (eftb_sync,
 * eftb_get, eftb_fetch_*) returns non-zero, naming the cosmology.  The reference has no such check: NaNs propagate silently there. */

/* Host <-> device state.  `offset`/`count` are in elements (doubles). */
int  eftb_put(eftb_engine* e, int buffer_id, size_t offset, const double* host, size_t count);
int  eftb_get(eftb_engine* e, int buffer_id, size_t offset, double* host, size_t count);
size_t eftb_buffer_size(const eftb_engine* e, int buffer_id); /* elements */

/* Launch the selected stages for cosmologies [0, B) (asynchronous; every other entry point orders itself behind it).
 * A full pipeline run spreads over three streams so that consecutive runs overlap: the front half (first stage .. expansions)
 * of run i+1 and the back half (spline, AP, projection, likelihood, reduce) of run i execute beside the resummation.
 * Environment switches, read by eftb_create: EFTB_PREP_OVERLAP=0 / EFTB_AP_OVERLAP=0 put the front / back half back on
 * the main stream (results are bit-identical either way). */
int  eftb_run(eftb_engine* e, int stage_mask, int B);
int  eftb_sync(eftb_engine* e);
/* Same, bracketed by HIP events on the engine stream; *ms receives the elapsed device time. */
int  eftb_run_timed(eftb_engine* e, int stage_mask, int B, int repeats, float* ms);

/* One call = reference theory.py:557-585 for a batch: host inputs in, templates out.
 * templ is [B][nl][24][nx] (rows as EFTB_B_TEMPL; (nl, nx) = the pipeline operator's output shape, else (Nl, Nk));
 * plk [B][nl][nx] may be NULL, else bias must be [B][24]; templ may be NULL when plk is requested (P_l only: 12 KB instead
 * of 0.3 MB per cosmology over PCIe at Nl=3, Nk=512). */
int  eftb_eval_batch(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA,
                     const double* H, double* templ, const double* bias, double* plk);

/* One call = theory + likelihood for a batch of walkers: reference theory.py:557-609, then EFTLike.PNG/PG
 * (likelihood.py:483-549) and Marginalizable.marginalized_logp (marginal.py:79-140).  Host inputs in, one marginalised
 * log-posterior per walker out; nothing else crosses PCIe.  Needs eftb_set_likelihood (and the pipeline operator that
 * brings the templates to the data's shape).  rows is PACKED [B][nG+1][24] (eftpipe_amd.parambasis.gaussian_rows);
 * logp [B / ntr] (NaN where det F2 <= 0: the reference raises there); fullchi2 [B / ntr] and best [B / ntr][nG] may be NULL.
 * With with_nnlo the NNLO part of the rows is whatever EFTB_B_GROWSN holds (eftb_put it beforehand; zero-initialised). */
int  eftb_eval_logp_batch(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA, const double* H,
                          const double* rows, double* logp, double* fullchi2, double* best);

/* Many EFT parameter draws against the CURRENT template block (the fast / slow split of the reference: EFTLeafKernel produces the
 * bias-independent templates once per cosmology, theory.py:557-609, and EFTLeaf.calculate contracts them with the EFT parameters of each
 * call, theory.py:829-874; samplers drag / oversample those fast parameters at fixed cosmology).  The current block is what
 * eftb_get(EFTB_B_TEMPL) would return now (+ EFTB_B_TEMPLN with with_nnlo): left by a synchronous template-producing run (eftb_run,
 * eftb_eval_batch, eftb_eval_logp_batch) or by eftb_put.  Draws are grouped by walker: offsets[C + 1] (offsets[0] = 0, non-decreasing,
 * offsets[C] = N); walker c (template entries c*ntr ... c*ntr + ntr - 1) owns draws [offsets[c], offsets[c + 1]), possibly none.
 * Both calls are synchronous and order themselves behind earlier work (queued staged steps included), as eftb_get does.  They refuse when
 * offsets are malformed, when C * ntr exceeds the entries the block holds, or when the block holds no templates (the last run was a direct-P_l
 * run, EFTB_O_PLK_DIRECT, or a staged step has rotated the blocks since the last template-producing synchronous run / eftb_put).
 *
 * eftb_draws_logp: the marginalised log-posterior per draw (likelihood.py:483-549, marginal.py:79-140) of the likelihood set by
 * eftb_set_likelihood, whose data index must address the block's shape.  rows PACKED [N][ntr][nG+1][24] (the rows of the LOGP stage,
 * eftpipe_amd.parambasis.gaussian_rows per tracer), rows_nnlo [N][ntr][nG+1][3] or NULL (zeros; with_nnlo only); logp [N] (NaN where
 * det F2 <= 0), fullchi2 [N] and best [N][nG] may be NULL.  Per walker the Gram matrix W = A C^-1 A^T of the template columns and the data
 * row is built on the first call after the block, the likelihood or the tracers change and reused after that; a draw then costs
 * O(nG (24 ntr)^2), independent of the data-vector length.
 *
 * eftb_draws_reduce: P_l per draw (reduce_Plk, parambasis.py:128-136, of EFTLeaf.calculate): bias [N][ntr][24] (the EFTB_B_BIAS coefficients
 * per tracer), bias_nnlo [N][ntr][3] or NULL (with_nnlo only; NULL: zeros) -> plk [N][ntr][nl][nx], the same bits as the REDUCE stage of the
 * walker's entries.  Neither call touches the buffers of the runs (device memory for the draws grows on demand, freed by eftb_destroy). */
int  eftb_draws_logp(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* rows, const double* rows_nnlo, double* logp,
                     double* fullchi2, double* best);
int  eftb_draws_reduce(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* bias, const double* bias_nnlo, double* plk);

/* The same draw calls fed with EFT parameter values: the coefficient rows are built on the device from a draw recipe, so a draw costs
 * 8 P bytes of host-to-device traffic instead of its dense rows.  A recipe states every non-zero entry of the rows as a sum of monomials
 *     coef * f^fpow * theta[i] * theta[j] * theta[k]          (an index of -1: the factor 1)
 * of the draw's parameter vector theta[P] and the growth rate f of its walker's tracer entry (eftpipe_amd.parambasis.DrawRecipe compiles
 * them from the scalar row builders).  A term names its entry by (tracer, row, col): row 0 ... ng1 - 1; col 0 ... 23 the template rows,
 * 24 ... 26 the NNLO columns (with_nnlo engines only).  Limits: P <= 32, 1 <= ng1 <= 25, nterms <= 1024, fpow <= 6.
 *
 * eftb_set_draw_recipe validates every term, sorts the terms by (row, tracer, col, fpow, i, j, k) -- the order their sum is taken in, whatever
 * order they arrive in -- and uploads them.  kind 0: the recipe of eftb_draws_logp_params (ng1 must be nG + 1 of the likelihood at the time
 * of the call; eftb_set_likelihood and eftb_set_tracers drop it); kind 1: the recipe of eftb_draws_reduce_params (ng1 = 1; eftb_set_tracers
 * drops it).  nterms = 0 withdraws the recipe.
 *
 * eftb_draws_logp_params / eftb_draws_reduce_params: eftb_draws_logp / eftb_draws_reduce with theta [N][P] and f [C][ntr] in place of the rows;
 * walkers, offsets, the Gram cache, the refusals and the outputs are those of the rows calls.  No per-draw row array exists on the logp
 * path; the reduce path evaluates the recipe into the [N][ntr][24] coefficient buffer on the device and contracts it as eftb_draws_reduce
 * does.  Non-finite theta or f is refused before anything is copied. */
typedef struct eftb_draw_term {
    double  coef;
    int32_t tracer, row, col, fpow;
    int32_t i, j, k;  /* indices into theta, -1 for the factor 1 */
    int32_t reserved;
} eftb_draw_term;
int  eftb_set_draw_recipe(eftb_engine* e, int kind, int P, int ng1, int nterms, const eftb_draw_term* terms);
int  eftb_draws_logp_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                            double* fullchi2, double* best);
int  eftb_draws_reduce_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* plk);

/* eftb_draws_logp_params with d ln P / d theta from an adjoint pass on the device: grad [N][P] in the order of theta (required: the call
 * without it is eftb_draws_logp_params).  ln P is the marginalised log-posterior of marginal.py:79-140 (marginalized_logp): with F2, F1,
 * F0 as there, b = F2^-1 F1 and v = (1, b), chi2 = F0 - F1 b + [not Jeffreys] ln det(F2 / 2 pi) has
 *     d chi2 = v^T dG v + [not Jeffreys] tr(F2^-1 dG[1:,1:]),     G = R^ W R^^T (the Gram form of eftb_draws_logp),
 * so d chi2 / d R^ = 2 S H with S = v v^T + [not Jeffreys] blockdiag(0, F2^-1) and H = R^ W, taken at the non-zero entries of the recipe and
 * contracted with the derivative of the recipe's monomials.  eftb_set_draw_recipe (kind 0) differentiates the sorted terms itself and keeps
 * the derivative terms sorted by (parameter, entry, parent term) beside the recipe: whatever drops or replaces the recipe does the same to
 * them, and the order of every sum is fixed, whatever order the terms arrived in and however the draws are split over calls.
 * Walkers, offsets, the Gram cache and the refusals are those of eftb_draws_logp_params; logp, fullchi2 and best are its bits.  A draw
 * with det F2 <= 0 gets NaN in all P slots of grad, as in logp. */
int  eftb_draws_logp_grad_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                                 double* grad, double* fullchi2, double* best);

/* eftb_draws_logp_grad_params with d2 ln P / d theta d theta: hess [N][P][P], grad [N][P] (both required).  With K = F2^-1, D_p = d R^ / d theta_p,
 * G_p = D_p H^T + H D_p^T, G_pq = D_pq H^T + H D_pq^T + D_p W D_q^T + D_q W D_p^T and u_p = (G_p v)[1:],
 *     d2 chi2 / d theta_p d theta_q = sum_gh S[g][h] G_pq[g][h] - 2 u_p^T K u_q - [not Jeffreys] tr(K G_p[1:,1:] K G_q[1:,1:])
 * (the middle term is the Schur complement of profiling b; the prior terms do not move), and d2 ln P = -1/2 of that.  eftb_set_draw_recipe
 * (kind 0) differentiates its sorted terms a second time itself and keeps those records, sorted by (p, q, entry, parent term) with p <= q,
 * beside the first-derivative table: whatever drops or replaces the recipe does the same to both.  The order of every sum depends on
 * the recipe alone, however the draws are split over calls; entry (q, p) is a copy of (p, q).  Walkers, offsets, the Gram cache and the
 * refusals are those of eftb_draws_logp_grad_params; logp, grad, fullchi2 and best are its bits.  A shape whose working set does not fit
 * the LDS with one wave per workgroup is refused (the message names P, nG and J + 1).  A draw with det F2 <= 0 gets NaN in all P^2 slots
 * of hess, as in grad and logp.  Nothing is iterated on the device: a Newton step on the host is eftpipe_amd.marginal.newton_maximize. */
int  eftb_draws_logp_hess_params(eftb_engine* e, int C, long long N, const int64_t* offsets, const double* theta, const double* f, double* logp,
                                 double* grad, double* hess, double* fullchi2, double* best);

/* Many data vectors sharing one covariance (mock realisations, pipeline validation, coverage tests), scored against the same templates.
 * A data set is one of M vectors data[M][ndata]; all share the index, invcov, priors and Jeffreys switch of the likelihood set by
 * eftb_set_likelihood, which must come first.  Only the last row and column of the Gram matrix W depend on the data: with U = A C^-1 of the
 * walker's template columns (eftb_draws_logp) and Ud = data C^-1,
 *     W[j][J] = W[J][j] = -(A_j . Ud_m + U_j . d_m) / 2,     W[J][J] = d_m . Ud_m,     W[:J][:J] as for the likelihood's own vector.
 * eftb_set_likelihood_datasets uploads the data sets and computes Ud once (the multiplication eftb_draws_logp applies to A); M = 0 withdraws
 * them, and eftb_set_likelihood and eftb_set_tracers drop them, as they drop the kind-0 recipe.  Non-finite data is refused before anything is
 * copied.  The LOGP stage, eftb_eval_logp_batch and the rows call eftb_draws_logp keep the likelihood's one vector. */
int  eftb_set_likelihood_datasets(eftb_engine* e, int M, const double* data);
/* eftb_draws_logp_params, eftb_draws_logp_grad_params (grad != NULL) or eftb_draws_logp_hess_params (grad and hess != NULL; hess needs grad)
 * per GROUP instead of per walker: group g = (walker[g] in [0, C), dataset[g] in [0, M)) owns the draws [offsets[g], offsets[g + 1]),
 * possibly none; offsets[G + 1] as for the walkers of the other calls.  Groups come in any order and may repeat a walker or a data set.
 * theta [N][P]; f [C][ntr] stays per walker.  Per group the (J + 1)^2 matrix Wg = the walker's W with the border of its data set is built by
 * one small kernel (8 (J + 1)^2 bytes per group, grown on demand; 2 (J + 1) dot products of length ndata) and kept until the template block,
 * the likelihood, the tracers, the data sets or the group table (walker, dataset) change; the kernels, records, outputs and refusals are those
 * of the three params calls.  A group whose data set equals the likelihood's own vector bit for bit returns the bits of those calls.  Refused,
 * naming the index: a walker outside [0, C) or beyond the template block, a data set outside [0, M), a call with no data sets set.  The
 * Gram cache of the other draw calls is shared, not disturbed: they return the same bits before and after. */
int  eftb_draws_logp_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, const int64_t* offsets,
                                     const double* theta, const double* f, double* logp, double* grad, double* hess, double* fullchi2, double* best);

/* Samples of the marginalised parameters of params draws, and what follows from them.  Given theta the marginalised parameters are exactly
 * Gaussian, b | theta, data ~ N(b^ = F2^-1 F1, F2^-1), with and without Jeffreys (which only drops ln det F2 from the marginal).  Per draw
 * the kernel runs the forward pass and solve of eftb_draws_logp_params (the same functions: logp, fullchi2 and best are that call's bits),
 * takes the upper Cholesky factor F2 = U^T U wave-synchronously without pivoting, and for each of the S standard-normal vectors
 * z [N][S][nG] of the caller returns
 *     bsamp [N][S][nG]      b = b^ + U^-1 z            (cov = U^-1 U^-T = F2^-1; z = 0 gives best bit for bit)
 *     chi2samp [N][S]       the full chi2 at b, by the formula and in the order of fullchi2 (z = 0: its bits)
 *     coef [N][S][ntr][24]  (or NULL) the coefficient rows R^[0] + sum_g b[g - 1] R^[g] of eftb_draws_reduce, from the entries of the kind-0
 *                           recipe in table order; coefn [N][S][ntr][3] (or NULL; with_nnlo engines only) their NNLO columns
 *     plk [N][S][ntr][nl][nx] (or NULL) P_l of every sample: draws_reduce_kernel launched as eftb_draws_reduce launches it on the N S
 *                           coefficient rows with offsets S -- the bits of eftb_draws_reduce fed with coef (and coefn); the rows then
 *                           stay on the device unless coef is given too
 * z comes from the caller: as many bytes as b going back, reproducible under any seed and stream discipline; there is no generator on
 * the device.  A sample's bits depend neither on S, nor on its place among the S, nor on how the draws are split into calls.
 * A draw whose F2 is not positive definite (a Cholesky pivot <= 0 or NaN) or has det F2 <= 0 gets NaN in all its samples, their chi2 and
 * coefficient rows (P_l follows); its record is what eftb_draws_logp_params returns for it.
 * Refused before anything is copied: what eftb_draws_logp_params refuses, S < 1, a non-finite z (naming draw, sample and parameter), coefn
 * on an engine without with_nnlo, a working set that does not fit the LDS (as eftb_draws_logp_params, plus 4 nG doubles per wave). */
int  eftb_draws_sample_params(eftb_engine* e, int C, long long N, int S, const int64_t* offsets, const double* theta, const double* f, const double* z,
                              double* logp, double* fullchi2, double* best, double* bsamp, double* chi2samp, double* coef, double* coefn, double* plk);
/* eftb_draws_sample_params per group (walker[g], dataset[g]) of eftb_draws_logp_params_datasets: the same kernel on the groups' Gram matrices.
 * No plk: draws_reduce_kernel addresses templates by walker; feed coef to eftb_draws_reduce walker by walker. */
int  eftb_draws_sample_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int S,
                                       const int64_t* offsets, const double* theta, const double* f, const double* z, double* logp, double* fullchi2,
                                       double* best, double* bsamp, double* chi2samp, double* coef, double* coefn);

/* Metropolis chains over the parameters theta of the kind-0 recipe at fixed templates: all T steps of all N chains in the kernel, one wave per
 * chain, so that a dragging or oversampling run pays one call instead of T.  Chain n belongs to the walker (or group) that owns draw n in
 * offsets, starts at theta0[n] and targets
 *     ln pi(theta) = ln P_marg(theta) + pri(theta),      pri = -1/2 sum_p ((theta_p - prior_loc_p) / prior_scale_p)^2 inside [lower, upper],
 * ln P_marg being the record of eftb_draws_logp_params (the same functions: every ln P, full chi2 and best fit of a chain are that call's
 * bits at that theta).  lower / upper [P] (NULL or -inf / inf: no bound) and prior_loc / prior_scale [P] (NULL or scale = inf: none) are
 * the sampler's prior on theta.  Nothing random happens on the device: the caller supplies step [N][T][P], the proposal increments
 * already multiplied by its proposal factor, and lnu [N][T], the logarithms of its uniforms (-inf allowed).  Step t of chain n:
 *     theta' = theta + step[n][t]; outside the box: rejected without an evaluation; otherwise the forward pass and solve at theta', and
 *     accepted iff ln P' is finite and lnu[n][t] < (ln P' + pri') - (ln P + pri)         (det F2 <= 0 at theta': rejected, no error)
 * pri is summed in parameter order as q = (theta_p - loc_p) sinv_p, acc = acc + q q, pri = -acc / 2 with sinv_p = 1 / scale_p (sinv_p = 0
 * skipped), every operation rounded on its own, and the accept expression is evaluated as written: NumPy reproduces both bit for bit.
 * After every thin-th step the state is stored: with K = T / thin,
 *     chain [N][K][P]       theta after steps thin, 2 thin, ...
 *     logp [N][K], fullchi2 [N][K], best [N][K][nG]   (each or NULL) the record at the stored theta
 *     last [N][P]           theta after step T (whether or not thin divides T): theta0 of the call that continues the chain
 *     naccept [N]           accepted steps
 * The host splits T into launches of at most 256 steps; between them only theta and the accept counts persist on the device and every
 * launch first recomputes the record of its starting theta, so a T-step call equals a T1-step call followed by a T2-step call from
 * `last` bit for bit, the accept counts summed (and the stored states too where thin divides T1).  A chain's bits do not depend on the
 * other chains of the call or on how the chains are split into calls.
 * A chain whose theta0 has no finite ln P (det F2 <= 0) fails alone: NaN in its chain, logp, fullchi2, best and last, naccept = -1.
 * Refused before anything is copied, naming chain, step and parameter where they apply: what eftb_draws_logp_params refuses, T < 1, thin
 * outside [1, T], a non-finite step, lnu NaN or > 0, lower > upper, a NaN bound, prior_scale <= 0 or NaN, theta0 outside the box, a working
 * set that does not fit the LDS (as eftb_draws_logp_params, plus 128 doubles per workgroup and 116 per wave). */
int  eftb_draws_chain_params(eftb_engine* e, int C, long long N, int T, int thin, const int64_t* offsets, const double* theta0, const double* f,
                             const double* step, const double* lnu, const double* lower, const double* upper, const double* prior_loc,
                             const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept);
/* eftb_draws_chain_params per group (walker[g], dataset[g]) of eftb_draws_logp_params_datasets: the same kernel on the groups' Gram matrices. */
int  eftb_draws_chain_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int T, int thin,
                                      const int64_t* offsets, const double* theta0, const double* f, const double* step, const double* lnu,
                                      const double* lower, const double* upper, const double* prior_loc, const double* prior_scale, double* chain,
                                      double* logp, double* fullchi2, double* best, double* last, int64_t* naccept);

/* Parallel tempering over theta at fixed templates: nlad ladders of R chains ("rungs") at the inverse temperatures beta [R],
 * 1 >= beta[0] > beta[1] > ... > beta[R - 1] >= 0, all T steps and every exchange between rungs in the kernel, one workgroup of R waves per
 * ladder.  The N = nlad R chains are counted by offsets as in eftb_draws_chain_params; chain n is rung n % R of ladder n / R, and every
 * walker's (group's) count is a multiple of R, so that no ladder straddles two walkers.  Rung r targets
 *     ln pi_r(theta) = beta[r] ln P_marg(theta) + pri(theta)
 * with ln P_marg the record of eftb_draws_logp_params, tempered as a whole -- it contains the Gaussian priors of the marginalised parameters,
 * which are therefore tempered with it -- and pri the chain call's prior on theta (box and independent Gaussians, the same arithmetic),
 * which is not.  Step i of the call is global step g = first_step + i:
 *     within a rung   the chain call's step: theta' = theta + step[n][i]; outside the box: rejected without an evaluation; otherwise accepted
 *                     iff ln P' is finite and lnu[n][i] < (beta[r] ln P' + pri') - (beta[r] ln P + pri), every operation rounded on its own.
 *                     beta[r] = 1: the products are exact, and a rung that never swaps is eftb_draws_chain_params' chain bit for bit
 *     swap event      after step i if (g + 1) % S == 0, event j = (g + 1) / S - 1 counted from the chain's beginning: the pairs (r, r + 1) with
 *                     r = j mod 2 and r + 1 < R are tried.  x = (beta[r] - beta[r + 1]) (ln P_{r+1} - ln P_r), two differences and a product,
 *                     each rounded; accepted iff lnu_swap[ladder][j_local][r] < x (-inf: always), where j_local counts the call's events from 0.
 *                     lnu_swap is [nlad][nsw][R - 1] with nsw = (first_step + T) / S - first_step / S (integer divisions); the entries of
 *                     the pairs an event does not try are not read.  On acceptance the two rungs exchange theta, the record (ln P, full
 *                     chi2, best fit) and pri; temperatures, naccept and sum_logp stay with the rung.  S = 0: no swaps (lnu_swap may be NULL)
 *     then            sum_logp[n] = sum_logp[n] + ln P of rung n's current state (untempered): a sequential sum of T terms, <ln P> at
 *                     beta[r] times T, what thermodynamic integration asks for; and after every thin-th step of the call (thin does not
 *                     look at first_step) the state is stored
 * Outputs, with K = T / thin:
 *     chain [N][K][P], logp [N][K], fullchi2 [N][K], best [N][K][nG] (the last three each or NULL), last [N][P], naccept [N]
 *                           as eftb_draws_chain_params; the records are untempered, the bits of eftb_draws_logp_params at the stored theta
 *     nswap [nlad][max(R - 1, 1)]   accepted swaps of every adjacent pair
 *     sum_logp [N]
 * A T-step call equals a T1-step call at first_step = s and a T2-step call at first_step = s + T1 from `last`, with step, lnu and lnu_swap
 * split accordingly, bit for bit in chain, records and last, naccept and nswap summed; sum_logp starts anew in every call and is not
 * claimed to combine.  The host splits T into launches of at most 256 steps; theta, naccept, nswap and sum_logp persist on the device
 * between them and every launch recomputes the records of its starting states.  A ladder's bits depend neither on the other ladders of
 * the call nor on their order.
 * A ladder one of whose rungs starts without a finite ln P (det F2 <= 0) fails as a whole: NaN in chain, logp, fullchi2, best, last and
 * sum_logp of every rung, naccept = nswap = -1; the other ladders are not touched.
 * Refused before anything is copied, naming ladder, rung, step or parameter where they apply: what eftb_draws_chain_params refuses, R
 * outside [1, 8], a walker whose chain count is no multiple of R, beta NaN, outside [0, 1] or not strictly decreasing, S < 0, first_step < 0,
 * a read entry of lnu_swap NaN or > 0, lnu_swap NULL with nsw > 0 and R > 1, and an R that does not fit the LDS: the chain call's working
 * set at R waves plus 40 doubles for the exchange, 320 bytes, within 160 KB (the message names R, the waves that fit, J + 1, nG and P). */
int  eftb_draws_temper_params(eftb_engine* e, int C, long long N, int R, int T, int S, long long first_step, int thin, const int64_t* offsets,
                              const double* theta0, const double* f, const double* beta, const double* step, const double* lnu, const double* lnu_swap,
                              const double* lower, const double* upper, const double* prior_loc, const double* prior_scale, double* chain, double* logp,
                              double* fullchi2, double* best, double* last, int64_t* naccept, int64_t* nswap, double* sum_logp);
/* eftb_draws_temper_params per group (walker[g], dataset[g]) of eftb_draws_logp_params_datasets: the same kernel on the groups' Gram matrices. */
int  eftb_draws_temper_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int R, int T, int S,
                                       long long first_step, int thin, const int64_t* offsets, const double* theta0, const double* f, const double* beta,
                                       const double* step, const double* lnu, const double* lnu_swap, const double* lower, const double* upper,
                                       const double* prior_loc, const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best,
                                       double* last, int64_t* naccept, int64_t* nswap, double* sum_logp);

/* Affine-invariant ensembles over theta at fixed templates (the stretch move of Goodman & Weare 2010, as in emcee): nens ensembles of K
 * members each, all T sweeps in the kernel, one workgroup per ensemble.  An ensemble takes the scale and orientation of its proposals from
 * its own members, so the call needs no proposal matrix.  The N = nens K chains are counted by offsets as in eftb_draws_chain_params; chain
 * n is member n % K of ensemble n / K, and every walker's (group's) count is a multiple of K, so that no ensemble straddles two walkers.
 * K is even, 2 <= K <= 64; members 0 ... K/2 - 1 are half 0, the rest half 1.  The target is the chain call's,
 *     ln pi(theta) = ln P_marg(theta) + pri(theta),
 * pri its prior on theta (box and independent Gaussians, the same arithmetic).  Sweep t = 0 ... T - 1 moves half 0 against the current
 * positions of half 1, then half 1 against the new positions of half 0.  Member k (chain n) moves as
 *     partner      j = member pick[n][t] of the other half, 0 <= pick < K/2       (pick [N][T], int32)
 *     proposal     per parameter d = theta_k - theta_j, theta' = theta_j + z[n][t] d, each operation rounded on its own     (z [N][T] > 0)
 *     box          outside the box: rejected without an evaluation
 *     acceptance   otherwise accepted iff ln P' is finite and lnq[n][t] < (ln P' + pri') - (ln P + pri), the chain call's expression
 * The caller folds the Jacobian of the stretch into its uniform, lnq = ln u - (P - 1) ln z: the device takes no logarithm.  lnq may
 * therefore be positive; -inf accepts every finite proposal.  After every thin-th sweep every member's state and record are stored.
 * Outputs, with Kt = T / thin: chain [N][Kt][P], logp [N][Kt], fullchi2 [N][Kt], best [N][Kt][nG] (the last three each or NULL), last [N][P]
 * and naccept [N] as eftb_draws_chain_params; every record is the bits of eftb_draws_logp_params at the stored theta.
 * A T-sweep call equals a T1-sweep call and a T2-sweep call from `last`, with z, pick and lnq split accordingly, bit for bit, naccept
 * summed.  The host splits T into launches of at most 256 sweeps; theta and naccept persist on the device between them and every launch
 * recomputes the records of its starting states.  An ensemble's bits depend neither on the other ensembles of the call nor on their order.
 * An ensemble one of whose members starts without a finite ln P (det F2 <= 0) fails as a whole: NaN in chain, logp, fullchi2, best and
 * last of every member, naccept = -1; the other ensembles are not touched.
 * Refused before anything is copied, naming ensemble, member, sweep or parameter where they apply: what eftb_draws_chain_params refuses but
 * for its rules on step and lnu, K odd or outside [2, 64], a walker whose chain count is no multiple of K, z NaN, infinite or <= 0, pick
 * outside [0, K/2), lnq NaN or +inf, and a K whose states leave no room for one wave: the chain call's working set at W waves plus 61
 * doubles per member within 160 KB, W = min(8, K/2, the waves that fit) (the message names K, J + 1, nG and P). */
int  eftb_draws_ensemble_params(eftb_engine* e, int C, long long N, int K, int T, int thin, const int64_t* offsets, const double* theta0, const double* f,
                                const double* z, const int32_t* pick, const double* lnq, const double* lower, const double* upper, const double* prior_loc,
                                const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept);
/* eftb_draws_ensemble_params per group (walker[g], dataset[g]) of eftb_draws_logp_params_datasets: the same kernel on the groups' Gram matrices. */
int  eftb_draws_ensemble_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int K, int T, int thin,
                                         const int64_t* offsets, const double* theta0, const double* f, const double* z, const int32_t* pick,
                                         const double* lnq, const double* lower, const double* upper, const double* prior_loc, const double* prior_scale,
                                         double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept);

/* Dragging chains between two cosmologies in one device call (the fast steps of cobaya's `drag: true` behind one slow proposal): the
 * chain call against a target that slides from a start walker to an end walker.  C walkers are resident, each with its own templates and
 * f [C][ntr]; pair g = (a = wstart[g], b = wend[g]) of G pairs (walkers may repeat, a = b is allowed) owns the chains
 * offsets[g] ... offsets[g + 1] - 1 (offsets [G + 1]).  With ln pi_x(theta) = ln P_x(theta) + pri(theta), ln P_x the record of
 * eftb_draws_logp_params for walker x and pri the chain call's prior on theta, step t = 0 ... T - 1 of chain n targets
 *     ln pi_t = (1 - frac[t]) ln pi_a + frac[t] ln pi_b          (frac [T], each in [0, 1]: the caller's schedule, t / (T + 1) for dragging)
 * Start: the records of theta0 at a and b and pri0; either ln P not finite: the chain fails as in the chain call (NaN everywhere, the sums
 * included, naccept = -1).  Otherwise sa = la0 + pri0, sb = lb0 + pri0.  Step t: theta' = theta + step[n][t]; outside the box: rejected
 * without an evaluation; otherwise la1 at a, lb1 at b (skipped where la1 is not finite), pri1, and with every operation rounded on its own
 *     u = 1 - frac[t];  a1 = la1 + pri1;  b1 = lb1 + pri1;  a0 = la0 + pri0;  b0 = lb0 + pri0;  w1 = u a1 + frac[t] b1;  w0 = u a0 + frac[t] b0
 *     accepted iff la1 and lb1 are finite and lnu[n][t] < w1 - w0
 * then, whatever the decision, sa = sa + (la0 + pri0) and sb = sb + (lb0 + pri0) with the current values.  NumPy reproduces all of it bit
 * for bit.  After every thin-th step the state and both current records are stored (thin = 0: no trajectory); with K = thin ? T / thin : 0
 *     chain [N][K][P]                 theta after steps thin, 2 thin, ... (may be NULL with thin = 0)
 *     logp_start, logp_end [N][K + 1], fullchi2_start, fullchi2_end [N][K + 1], best_start, best_end [N][K + 1][nG]   (each or NULL)
 *                                     the records at the stored theta for a and for b, and in slot K those of the state after step T
 *     last [N][P], naccept [N]        as the chain call
 *     sums [N][2]                     sa, sb: T + 1 terms each; (sb - sa) / (T + 1) is the logarithm of the acceptance ratio of the whole
 *                                     slow + fast move when frac[t] = (t + 1) / (T + 1)
 * Every ln P, full chi2 and best fit is the bit pattern of eftb_draws_logp_params for that (walker, theta).  The host splits T into launches
 * of at most 256 steps; theta, the accept counts and the sums persist on the device between them and every launch recomputes both
 * starting records, so a chain's bits depend neither on the split nor on the other chains, pairs or their order.
 * Each workgroup stages both walkers' Gram matrices: 2 (J + 1)^2 doubles beside at least one wave's scratch in 160 KB, which holds up to
 * three tracers with NNLO (J + 1 = 82) at nG = 24; four tracers at nG = 24 and five tracers at any nG are refused.
 * Refused before anything is copied, naming pair, chain, step or parameter: what eftb_draws_chain_params refuses (thin outside [0, T]
 * here), a pair's walker outside [0, C), NaN or a value outside [0, 1] in frac, and a shape that does not fit the LDS (the message names
 * J + 1 and nG and says that the call stages two Gram matrices).  There is no data-set (groups) variant. */
int  eftb_draws_drag_params(eftb_engine* e, int C, int G, const int32_t* wstart, const int32_t* wend, long long N, int T, int thin, const int64_t* offsets,
                            const double* theta0, const double* f, const double* frac, const double* step, const double* lnu, const double* lower,
                            const double* upper, const double* prior_loc, const double* prior_scale, double* chain, double* logp_start, double* logp_end,
                            double* fullchi2_start, double* fullchi2_end, double* best_start, double* best_end, double* last, int64_t* naccept,
                            double* sums);

/* Hamiltonian Monte Carlo over the draw parameters in one device call: the chain call with leapfrog trajectories in the place of its
 * random-walk steps.  Walkers, offsets, theta0, f, the target ln pi = ln P_marg + pri, the box and the prior on theta are the chain
 * call's.  The caller supplies all randomness and all tuning: mom [N][T][P] (standard normals), lnu [N][T] (logarithms of uniforms, -inf
 * allowed), eps [N][T] (the step size of every trajectory), nleap (leapfrog steps per trajectory, one value for the call) and factor
 * [N][P][P] (or NULL: the identity), per chain a lower-triangular F with M^-1 = F F^T of which only the lower triangle is read.  The
 * momenta live in the whitened space (kinetic energy r.r / 2).  With g = grad ln P_marg + grad pri, the first the bits of
 * eftb_draws_logp_grad_params and (grad pri)_p = -((theta_p - loc_p) sinv_p) sinv_p (sinv_p = 0 skipped), trajectory t of chain n is
 *     r = mom[n][t];  k = 1/2 sum_p r_p r_p;  h = 0.5 eps;  r = r + h u,  u_p = sum_{q >= p} F[q][p] g_q
 *     nleap times:  theta_p = theta_p + eps v_p,  v_p = sum_{q <= p} F[p][q] r_q;  the box test, then record and g at theta;
 *                   r = r + (eps, or h the last time) u
 *     ratio = ((ln P' + pri') - k') - ((ln P + pri) - k);  accepted iff the trajectory was not aborted and lnu[n][t] < ratio
 * all sums with the index ascending from 0 as acc = acc + x y, every operation rounded on its own: NumPy reproduces it bit for bit.  A
 * trajectory is aborted, and so rejected, when a position lies outside the box (no reflection, no evaluation there) or its ln P or a
 * component of g is not finite; that is no error.  After every thin-th trajectory the state is stored, as the chain call stores steps:
 *     chain [N][K][P], logp [N][K], fullchi2 [N][K], best [N][K][nG], last [N][P], naccept [N]     K = T / thin, as the chain call
 *     log_ratio [N][T] (or NULL)     ratio of every trajectory, NaN where it was aborted: what a step-size adaptation on the host needs
 * The host splits T into launches of max(1, 256 / nleap) trajectories; only theta and the accept counts persist between them and every
 * launch recomputes record and gradient of its start, so a T-trajectory call equals a T1 + T2 call from `last` bit for bit.  A chain whose
 * theta0 has no finite ln P fails alone: NaN in its outputs (log_ratio included), naccept = -1.
 * Refused before anything is copied, naming chain, trajectory and parameter where they apply: what eftb_draws_chain_params refuses (mom in
 * the place of step), nleap < 1 or > 256, an eps that is not finite and positive, a factor entry of the lower triangle that is not finite,
 * a diagonal entry <= 0, and a working set that does not fit the LDS (the chain call's plus the recipe's rows, 96 + P^2 doubles per wave;
 * the message names P, nG and J + 1): four tracers with NNLO at nG = 24 and 1024 recipe entries fit with P = 32, five tracers there do not. */
int  eftb_draws_hmc_params(eftb_engine* e, int C, long long N, int T, int nleap, int thin, const int64_t* offsets, const double* theta0, const double* f,
                           const double* mom, const double* lnu, const double* eps, const double* factor, const double* lower, const double* upper,
                           const double* prior_loc, const double* prior_scale, double* chain, double* logp, double* fullchi2, double* best, double* last,
                           int64_t* naccept, double* log_ratio);
/* eftb_draws_hmc_params per group (walker[g], dataset[g]) of eftb_draws_logp_params_datasets: the same kernel on the groups' Gram matrices. */
int  eftb_draws_hmc_params_datasets(eftb_engine* e, int C, int G, const int32_t* walker, const int32_t* dataset, long long N, int T, int nleap, int thin,
                                    const int64_t* offsets, const double* theta0, const double* f, const double* mom, const double* lnu, const double* eps,
                                    const double* factor, const double* lower, const double* upper, const double* prior_loc, const double* prior_scale,
                                    double* chain, double* logp, double* fullchi2, double* best, double* last, int64_t* naccept, double* log_ratio);

/* Pipelined sampler steps.  The per-step inputs (Pin, f, DA, H, bias rows, likelihood rows) and outputs (EFTB_B_PLK, EFTB_B_LOGP)
 * exist three times: one set is being evaluated, the next is already queued behind it, the third is being fetched from / refilled --
 *     eftb_stage_inputs(step i+1);  eftb_run_staged(step i+1);  eftb_fetch_previous(step i);   ...
 * nothing in this loop waits for the step in flight, so consecutive steps overlap on the GPU (the front half of step i+1 runs beside
 * the resummation / AP of step i) and the PCIe traffic hides behind the kernels.  The host arrays may be reused as soon as
 * eftb_stage_inputs returns (they are copied into page-locked staging memory).  bias ([B][24]) and rows (packed [B][nG+1][24])
 * may be NULL.  No reference counterpart (cobaya evaluates one point at a time). */
int  eftb_stage_inputs(eftb_engine* e, int B, const double* Pin, const double* f, const double* DA, const double* H,
                       const double* bias, const double* rows);
int  eftb_run_staged(eftb_engine* e, int stage_mask, int B);
/* (Round 4.)  A staged step handed in while earlier ones are still queued or running is only QUEUED by eftb_run_staged: the library's submission
 * thread issues it (EFTB_O_SUBMIT_THREAD), together with whatever else is queued by then if eftb_config.step_batch allows.  A launch error of such
 * a step cannot be returned by eftb_run_staged any more: the step still counts (`back` indices are positions in the sequence of steps handed in) and
 * the eftb_fetch_* call of THAT step returns the error; the same holds for a step the calling thread issued itself. */
/* EFTB_B_PLK or EFTB_B_LOGP of the step before the one in flight (waits only for that step). */
int  eftb_fetch_previous(eftb_engine* e, int buffer_id, double* host, size_t count);
/* The same for the step launched `back` (0 = the last one itself, 1 ... 15) steps before the last one.  The engine keeps sixteen sets of per-launch inputs / outputs, so the
 * loop  stage(i); run_staged(i); fetch_back(3) [= step i - 3]  keeps THREE steps queued on the GPU while the host copies results out and
 * prepares the next inputs: the inputs of step i + 1 are then staged before the back half of step i - 1 has finished, and the look-ahead
 * of consecutive steps never runs dry (with back = 2 the look-ahead stream idled ~0.1 ms per step waiting for the host).  Direct-P_l runs
 * (EFTB_O_PLK_DIRECT) are four pipeline stages deep -- front, syntheses + contraction, resummation, AP -- and want back = 4 or more; the set
 * read with back = 15 is the one the sixteenth launch from there refills. */
int  eftb_fetch_back(eftb_engine* e, int back, int buffer_id, double* host, size_t count);
/* The same results without the host copy: *block points at the engine's page-locked host copy of the step's EFTB_B_PLK / EFTB_B_LOGP block
 * (*count = its capacity in elements), valid until NSETS - 1 = 15 more steps have been staged.  For samplers that consume P_l in place (the
 * dependent loop of reference likelihood.py:570-594: chi^2 from P_l, then the next proposal). */
int  eftb_fetch_view(eftb_engine* e, int back, int buffer_id, const double** block, size_t* count);
/* The end of a burst: the steps queued so far leave now, in as few launches as eftb_config.step_batch allows, instead of waiting for more steps to
 * fill a launch (the submission thread lets the queue grow while two launches are in flight).  Returns at once; a sampler calls it before it
 * fetches the last steps of a batch of proposals (reference: the end of one Cobaya `Model.logposterior` sweep over the walkers). */
int  eftb_flush(eftb_engine* e);
/* Where the P_l of the staged step launched NEXT goes: the caller's own page-locked array (eftb_host_alloc / hipHostMalloc / hipHostRegister;
 * `count` doubles, at least B x Nl x Nx of the step's output) instead of the engine's host block -- the copy-out behind the step writes it with
 * the DMA engine, so a sampler that keeps every step's P_l (emulator training sets, the chains' derived output of cobaya's `output_params`,
 * reference theory.py:557-609 per point) pays no second host copy.  One step only; dst = NULL withdraws it.  eftb_fetch_view of that step
 * hands out dst once the step has finished (eftb_fetch_back copies from it); the array must stay allocated and untouched until then.  Refused:
 * pageable memory, engines with a communicator, runs that form no P_l (LOGP); an array that turns out too small for the step's rows fails the
 * launch, reported by the step's fetch.  May be called while earlier steps are queued (it does not wait for them). */
int  eftb_set_step_output(eftb_engine* e, double* dst, size_t count);
/* One sampler step in one call: eftb_stage_inputs + eftb_run_staged + (back >= 0 and that many steps already behind this one)
 * eftb_fetch_view(back, buffer_id).  *block stays NULL while the pipeline is still filling.  Replaces, per step of a batched sampler, what
 * EFTLeafKernel.calculate_power_spectrum + reduce_Plk do per point (theory.py:557-609, parambasis.py:42-136). */
int  eftb_step(eftb_engine* e, int stage_mask, int B, const double* Pin, const double* f, const double* DA, const double* H,
               const double* bias, const double* rows, int back, int buffer_id, const double** block, size_t* count);

/* Host-side cost of the staged steps, for bench.py's accounting (measurement only): enable != 0 switches the clocks on; out (may be NULL) receives
 * {steps issued, of which by the caller's thread, us spent issuing (upload kernel + launches + events, whichever thread), us spent copying inputs
 * into the staging blocks, us the caller spent waiting for results in eftb_fetch_*, launches that carried those steps}; reset != 0 clears the sums. */
int  eftb_submit_stats(eftb_engine* e, int enable, int reset, double out[6]);

/* The last (up to 64) traced launches (EFTB_O_STEP_TRACE), oldest first: out[i][0] = launch number, out[i][1] = cosmologies it carried, out[i][2..13] = the
 * twelve timestamps (the nine of EFTB_O_STEP_TRACE, then upload end, first-stage products end, anti-diagonal sums end) in microseconds since the option was switched on (-1000: point not recorded).  Waits for everything in flight. */
int  eftb_step_trace(eftb_engine* e, double* out, int max_launches, int* n_out);

/* Page-locked host memory for the I/O buffers of eftb_eval_batch / eftb_put / eftb_get: D2H of the template block runs at
 * the PCIe rate instead of through the driver's pageable staging copy.  NULL on failure (eftb_last_error). */
void* eftb_host_alloc(size_t bytes);
void  eftb_host_free(void* p);

/* Multi-GPU: cosmologies are sharded over ranks (one process per GPU); the only exchange is the gather of
 * the per-cosmology P_l(k) to `root` over RCCL (xGMI).  No reference counterpart: cobaya chains are
 * independent MPI processes (reference README.md:29-34).  The 128-byte id comes from rank 0
 * (eftb_comm_unique_id) and is handed to every rank by the host (any side channel). */
int  eftb_comm_unique_id(char id[128]);
int  eftb_comm_init(eftb_engine* e, int nranks, int rank, const char id[128]);
/* Gather EFTB_B_PLK rows [0, B) of every rank into root's device buffer (rank-major), in line behind the kernel that
 * wrote them (on the back-half stream of an overlapped run, else on the compute stream);
 * if host_out != NULL (root only) the gathered block [nranks][B][Nl][Nx] is copied out after the gather. */
int  eftb_gather_plk(eftb_engine* e, int B, int root, double* host_out);
/* Pipelined multi-GPU steps (eftb_stage_inputs / eftb_run_staged / eftb_gather_plk per step, nothing waits for the step in flight): on the
 * root the gathered block rotates through four device buffers, and each is copied on to page-locked host memory by a copy kernel on its own
 * stream as soon as its exchange has finished -- 12.6 MB per step at 8 ranks, which a blocking device-to-host copy into pageable memory would
 * turn into the bottleneck of the whole node.  eftb_fetch_gathered copies the block ([nranks][B][nl][nx], count elements) of the last exchange
 * enqueued (back = 0) or of the one `back` (1 ... 3) exchanges before it into `host`, waiting only for that exchange; eftb_gathered_view hands
 * out the page-locked block itself instead (no host copy; valid until three more exchanges have been enqueued).  With a communicator
 * (eftb_comm_init, to be called before the first eftb_stage_inputs) the staged sets keep P_l in device memory, where RCCL reads it. */
int  eftb_fetch_gathered(eftb_engine* e, int back, double* host, size_t count);
int  eftb_gathered_view(eftb_engine* e, int back, const double** block, size_t* count);

/* Window precompute (reference Window._compute_Wal / _compute_Waldk, window.py:262-359) on the device.  The caller passes
 * the k-independent tables of eftpipe_amd.tables.window_tables: x [nx] (FFTLog samples inside the tabulated window), Qt
 * [Na][Nl][nx] (Q_al(x) with the FFTLog tilt and (-1)^a), T [Nl][nx][Np] (FFT + power-law sum collapsed per l) and the p grid;
 *   Wal [Na][Nl][Nk][Np]  = sum_i Qt_al[i] j_{2a}(k x_i) T_l[i][p]                (the reference's *.npy cache content)
 *   Waldk (optional)      = Wal * [|p - k| < windowk, if withmask] * dp            (window.py:348-359)
 *   Wfold (optional, needs S [Np][Nk], the k -> p cubic-spline matrix) = Waldk S  [Na][Nl][Nk][Nk], what Window.Window applies.
 * All pointers are host buffers, C-contiguous float64; device_ms (optional) receives the kernel time without the copies. */
int  eftb_window_precompute(int device, int Na, int Nl, int Nk, int nx, int Np, const double* k, const double* x,
                            const double* Qt, const double* T, const double* p, int withmask, double windowk,
                            const double* S, double* Wal, double* Waldk, double* Wfold, double* device_ms);

/* Measured FP64 MFMA issue rate (v_mfma_f64_16x16x4_f64), TFLOP/s, for the roofline denominator. */
int  eftb_mfma_f64_peak(int device, double* tflops);

/* Counter calibration: one kernel that streams `bytes` of device memory once with 8 or 16 bytes per lane (two launches; the second is
 * timed).  Run under `rocprofv3 --pmc FETCH_SIZE` it tells how the counter tallies each access width (tools/fetch_calib.py). */
int  eftb_stream_read_probe(int device, size_t bytes, int bytes_per_lane, double* gbps);

const char* eftb_last_error(void);
const char* eftb_version(void);
/* first 16 hex digits of sha256(eftbird.hip + eftb_kernels.hpp + eftb_staged.hpp + eftb_own.hpp) of the build (csrc/Makefile); the key of csrc/isa_counts.json */
const char* eftb_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* EFTBIRD_H */
