// tcfd_ns2d_plan.hpp -- internal header of the spectral solver's translation units: the plan, the workspace layouts and the
// entry points of the size-templated kernels.
//   tcfd_ns2d.hip         the C ABI: plans, argument checks, chunking, the size-free kernels
//   tcfd_ns2d_sized.hip   every kernel templated on the grid size, its launchers and drivers; built once per real type
//   tcfd_ns2d_refine.hip  the spectral refiner on top of the two
#pragma once
#include <mutex>
#include <vector>

#include "tcfd_fft.hpp"
#include "tcfd_host.hpp"

using tcfd::cx;

#define fail(...) FAIL(__VA_ARGS__)

// Every grid size the solver is instantiated for: 2^k, 3 * 2^k and 5 * 2^k.  plan_create's check and the sized units' switch
// over n are generated from this list; the tile parameters of a size are its Cfg rows in tcfd_ns2d_sized.hip.
#define TCFD_NS2D_SIZES(X)                                                                          \
    X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(96) X(192) X(384) X(768) \
    X(80) X(160) X(320) X(640) X(1536) X(1280)

// ------------------------------------------------------------------ plan
struct ProfRec { int kind; hipEvent_t e0, e1; };
struct ProfState {
    bool on = false;
    int max_records = 0;
    std::vector<ProfRec> recs;
};

// hipGraph of ONE interior RK step (nstages x {row pass, fused column pass}, state upad -> upad): for small grids a
// step is 10 launches of 7-20 us each and launch gaps are a quarter of the time; a steps=k call replays the graph
// for its k-2 interior steps on a plan-owned stream (capture is not allowed on the legacy default stream PyTorch
// hands over), fenced by events against the caller's stream.
struct GraphState {
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipStream_t stream2 = nullptr;                 // batch-halves overlap (TCFD_OVERLAP): second lane
    hipEvent_t ev_out2 = nullptr, ev_rows = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    // the same step MULTI times in one graph: a graph launch costs ~10 us of idle device between replays, a sixth
    // of a 256^2 step; long calls replay this one and finish with the single-step graph
    static constexpr int MULTI = 16;
    hipGraphExec_t exec_multi = nullptr;
    hipGraph_t graph_multi = nullptr;
    // key of the captured sequence
    long batch = -1;
    int nstages = 0;
    void* ws = nullptr;
    std::vector<double> coef;
    const void* ens = nullptr;   // the chunk's slice of the plan's ensemble table (null on a scalar plan)
};

// Tuning switches (environment, read ONCE at plan creation and frozen in the plan: two plans of one process may
// differ, a plan never changes its kernels behind the caller's back).  -1 = automatic.
struct Tuning {
    int split;               // TCFD_SPLIT: radix-2 split of the column transform across the row pass
    int small_tiles;         // TCFD_SMALL_TILES: 4-column tiles / 64-lane row groups for small problems
    int two_wg;              // TCFD_TWO_WG: 128-VGPR cap (two workgroups per CU) for the 512-point fp64 column tiles
    int f32_cols8;           // TCFD_F32_COLS8: fp32 512-point column tiles of 8 columns (64-byte segments, pairs on one XCD) on the
                             // cross-lane transforms for the plane-emitting passes (1 = default); 0 = 16-column Stockham tiles
    int nt_out;              // TCFD_NT_OUT: non-temporal stores of the last stage's outputs (new state to the caller, dw/dt)
    int cols_lds_pad;        // TCFD_COLS_LDS_PAD: extra dynamic LDS bytes of the column kernels (experiments)
    int rows7_minw;          // TCFD_ROWS7_MINW: waves per SIMD of the fp32 cross-lane row kernel (2 / 4)
    int rows_blocks_per_cu;  // TCFD_ROWS_BLOCKS_PER_CU: persistent row-pass grid
    int pair_xcd;            // TCFD_PAIR_XCD: put the 2 / 4 column tiles that share a 128-byte line on one XCD (0 off, 2 pairs only, 4 at most four, 8 always eight)
    int ablate;              // TCFD_ABLATE: timing ablations (results are WRONG when non-zero)
    int nt_planes;           // TCFD_NT_PLANES: non-temporal plane stores (-1: for the small-tile launches only)
    int rows_v;              // TCFD_ROWS_V: 0 = per size; 5 = register-staged rows with Stockham exchanges, 7 = cross-lane
                             // transforms (1024 points fp64 only).  (4 / 6 -- round 1's two-plane kernels, LDS-DMA staging --
                             // were removed in round 5; the values now mean 5)
    int cols_xl;             // TCFD_COLS_XL: cross-lane column transforms where available (1 = default)
    int nyq_pack;            // TCFD_NYQ_PACK: packed Nyquist column in the step (1 = default where the plan allows it)
    int chunk;               // TCFD_CHUNK: fields per chunk of a batched call (0 = whole batch at once, -1 = cache sized)
    int bundle_rows;         // TCFD_BUNDLE_ROWS: row pass of the tangent-bundle calls: -1 = per size (bundle_two_pass), 0 = the two-pass
                             // form of k_rows_jvp everywhere, 1 = k_rows_jvp_bundle wherever its stash fits a CU's LDS (A/B of the two)
    int graph;               // TCFD_GRAPH: hipGraph replay of interior steps (1 = on; off by default since round 4: plain stream
                             // launches measured 3-13 % faster than replay for every small problem, tests/micro/graph_crossover.py)
    int overlap;             // TCFD_OVERLAP: two half batches on two streams (opt-in experiment)
    int round_fields;        // n = 3 * 2^k: fields whose column tiles fill the resident workgroup slots exactly once (0: not used)
    size_t cache_bytes;      // last-level (Infinity Cache / MALL) size of the plan's device: what a chunk is sized for
    int cache_source;        // 0 = built-in 256 MB, 1 = KFD topology of this device, 2 = TCFD_CACHE_MB
};

struct tcfd_ns2d_plan {
    Tuning tune;
    std::mutex mu;    // guards the mutable side-cars below (the tables are immutable after creation)
    ProfState* prof;  // mutable side-car (tcfd_ns2d_profile_begin/end); null until first use
    GraphState* gs;   // mutable side-car: captured interior step (null until first use)
    int n, m, dtype;
    int ldw;        // workspace row pitch in elements: m rounded up so that a row is a multiple of 128 bytes
    void* tw;       // cx<T>[n]
    void* tw2;      // cx<T>[n/2]: table of the half-length column transforms (split plans)
    void* kx;       // T[n]
    void* ky;       // T[m]
    void* lin;      // T[n*m]
    void* mask;     // T[n*m]
    void* forcing;  // cx<T>[n*m] or null (dense form, used when the forcing is not sparse)
    // exact compact forms found at plan creation (the (n, m) tables cost ~2x the state's bytes per
    // column tile in L2 traffic; the reference's own tables are separable / sparse by construction)
    void* mask_r; void* mask_c; void* lin_r; void* lin_c;  // T[n], T[m], T[n], T[m]
    void* f_ptr; void* f_row; void* f_val; void* f_col;    // int[m+1], int[nnz], cx<T>[nnz], int[nnz]
    int f_nnz;
    int sep;        // mask and linear term are separable
    int f_sparse;   // forcing stored as CSC
    int nyq_a, nyq_ca;   // ... in the opening pass / in the fused passes of a step (set with nyq at plan creation)
    int nyq;        // packed Nyquist column in the step kernels (emit_planes): the plan is pruned (F = h = 0 in column
                    // m - 1), n >= 64 (every column tile width divides n / 2) and the row kernels are v5 / v7
    // per-sample physics (tcfd_ns2d_plan_set_ensemble; all null / 0 on a scalar plan, whose kernels then run as before)
    void* ens;      // T[4 * ens_count]: {nu, drag, forcing_scale, l00 = nu * lap[0][0] - drag} per field of a call
    long ens_count; // > 0: the plan steps ensembles of exactly this many fields
    void* lap;      // T[n*m] laplacian (uploaded only when the separable form is not used)
    void* lap_r; void* lap_c;   // T[n] its column 0, T[m] its row 0
    int ens_sep;    // every member's nu * lap - drag passes plan_fill's separability test (and the mask is separable)
    int keep_cols;  // > 0: F (hence the RK accumulator h) is identically zero for columns >= keep_cols and for
                    // rows with mask_r == 0 (2/3-rule mask, forcing inside the mask): those entries of the
                    // advection / h arrays are neither written nor read.  0: no pruning.
};

static size_t field_bytes(const tcfd_ns2d_plan* p, long batch) {
    const size_t esz = p->dtype == TCFD_C128 ? 16 : 8;
    return align256((size_t)batch * p->n * p->ldw * esz);
}

// ------------------------------------------------------------------ optional per-launch event timing
// kinds: 0 cols MODE_A, 1 rows_advect, 2 cols MODE_CA, 3 cols MODE_C (+ dw/dt), 5 other   (4 was the separate dw/dt pass)
struct ProfScope {
    ProfState* ps;
    hipStream_t st;
    int idx = -1;
    ProfScope(const tcfd_ns2d_plan* p, int kind, hipStream_t s) : ps(p->prof), st(s) {
        if (!ps || !ps->on || (int)ps->recs.size() >= ps->max_records) { ps = nullptr; return; }
        ProfRec r;
        r.kind = kind;
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) { ps = nullptr; return; }
        (void)hipEventRecord(r.e0, st);
        ps->recs.push_back(r);
        idx = (int)ps->recs.size() - 1;
    }
    ~ProfScope() {
        if (ps) (void)hipEventRecord(ps->recs[idx].e1, st);
    }
};

// ------------------------------------------------------------------ workspace layouts
template <typename T>
struct Ws {
    cx<T>* h;
    cx<T>* adv;
    cx<T>* planes;
    cx<T>* upad;          // state in the line-aligned internal pitch (stages 1.. of a call)
    cx<T>* upad2;         // intermediate state of schedules whose later stages restart from the step's initial state
    size_t plane_stride;  // elements
};
template <typename T>
static Ws<T> carve(const tcfd_ns2d_plan* p, void* ws, long batch) {
    const size_t fb = field_bytes(p, batch);
    unsigned char* base = (unsigned char*)ws;
    Ws<T> w;
    w.h = (cx<T>*)base;
    w.adv = (cx<T>*)(base + fb);
    w.planes = (cx<T>*)(base + 2 * fb);
    w.upad = (cx<T>*)(base + 6 * fb);
    w.upad2 = (cx<T>*)(base + 7 * fb);
    w.plane_stride = fb / sizeof(cx<T>);
    return w;
}

// Scratch of the tangent-linear calls: 16 chunk-sized fields -- two plane sets, two advection fields, h and dh, and the two
// intermediate states of the stepper for w and dw.
template <typename T>
struct JvpWs {
    cx<T>* planes;
    cx<T>* dplanes;
    cx<T>* adv;
    cx<T>* dadv;
    cx<T>* h;
    cx<T>* dh;
    cx<T>* s[2];          // intermediate states (caller layout, pitch m)
    cx<T>* ds[2];
    size_t plane_stride;  // elements
};
template <typename T>
static JvpWs<T> carve_jvp(const tcfd_ns2d_plan* p, void* ws, long batch) {
    const size_t fb = field_bytes(p, batch);
    unsigned char* base = (unsigned char*)ws;
    auto at = [&](int i) { return (cx<T>*)(base + (size_t)i * fb); };
    JvpWs<T> w;
    w.planes = at(0);
    w.dplanes = at(4);
    w.adv = at(8);
    w.dadv = at(9);
    w.h = at(10);
    w.dh = at(11);
    w.s[0] = at(12);
    w.ds[0] = at(13);
    w.s[1] = at(14);
    w.ds[1] = at(15);
    w.plane_stride = fb / sizeof(cx<T>);
    return w;
}

// Scratch of the tangent-BUNDLE calls (one state, K tangents; tcfd_ns2d_*_jvp_bundle): chunk-sized fields again.  The plane sets
// and advection fields exist for the state and for ONE GROUP of kg <= K tangents (the tangents pass through the sweep group by
// group: bundle_shape in tcfd_ns2d.hip); everything the stepper carries from stage to stage exists K times.  9 + 5 kg + 4 K fields.
// The group's planes are stored [plane][tangent][field]: `dplane_stride` apart per plane, `plane_stride` apart per tangent, so
// that ONE column launch over kg * batch fields fills or drains a group.  dF, dh and ds hold K tangents of batch fields each in
// the caller's pitch, tangent after tangent (`tan_stride` elements apart).
static inline int bundle_fields(int ntan, int kg) { return 9 + 5 * kg + 4 * ntan; }
template <typename T>
struct BundleWs {
    cx<T>* planes;        // 4: the state's planes
    cx<T>* dplanes;       // 4 kg
    cx<T>* adv;           // 1
    cx<T>* dadv;          // kg
    cx<T>* F;             // 1: F(u) of the stage (caller layout, pitch m)
    cx<T>* h;             // 1
    cx<T>* s[2];          // 2: intermediate states
    cx<T>* dF;            // K
    cx<T>* dh;            // K
    cx<T>* ds[2];         // K each
    size_t plane_stride;  // elements of one chunk-sized field
    size_t dplane_stride; // kg * plane_stride
    size_t tan_stride;    // batch * n * m
};
template <typename T>
static BundleWs<T> carve_bundle(const tcfd_ns2d_plan* p, void* ws, long batch, int ntan, int kg) {
    const size_t fb = field_bytes(p, batch);
    unsigned char* base = (unsigned char*)ws;
    auto at = [&](long i) { return (cx<T>*)(base + (size_t)i * fb); };
    BundleWs<T> w;
    long i = 0;
    w.planes = at(i); i += 4;
    w.dplanes = at(i); i += 4L * kg;
    w.adv = at(i); i += 1;
    w.dadv = at(i); i += kg;
    w.F = at(i); i += 1;
    w.h = at(i); i += 1;
    w.s[0] = at(i); i += 1;
    w.s[1] = at(i); i += 1;
    w.dF = at(i); i += ntan;
    w.dh = at(i); i += ntan;
    w.ds[0] = at(i); i += ntan;
    w.ds[1] = at(i);
    w.plane_stride = fb / sizeof(cx<T>);
    w.dplane_stride = (size_t)kg * w.plane_stride;
    w.tan_stride = (size_t)batch * p->n * p->m;
    return w;
}

// Scratch of the adjoint model (tcfd_ns2d_step_vjp): the 8 fields of `Ws` for the forward and the adjoint sweeps of the explicit
// terms (which touch `adv` and `planes` only), with the three fields those sweeps leave alone put to use, then 4 fields of X_f,
// the cotangent of the step's initial state and the recomputed stage states u_1 .. u_{nstages-1}: 12 + nstages fields.
constexpr int VJP_MAX_STAGES = 32;
static inline int vjp_fields(int nstages) { return 12 + nstages; }
template <typename T>
struct VjpWs {
    cx<T>* ubar;          // Ws::h: the running cotangent of the state, alive from one reversed step to the next
    cx<T>* F;             // plane 0 of Ws::planes: F(u_k) of the recomputation (the planes are dead after the row pass)
    cx<T>* hf[2];         // Ws::upad, Ws::upad2: the accumulator h of the recomputation, ping-pong ...
    cx<T>* gm;            // ... then (same fields, the recomputation is over) the pre-weighted cotangent of F
    cx<T>* hbar;          //     and the cotangent of h
    cx<T>* X;             // the four half spectra of explicit_vjp, `stride` apart
    cx<T>* ustart;        // cotangent of the step's initial state through the base0 stages
    cx<T>* u;             // u_1 .. u_{nstages-1}, `stride` apart
    size_t stride;        // elements per field
};
template <typename T>
static VjpWs<T> carve_vjp(const tcfd_ns2d_plan* p, void* ws, long batch) {
    const size_t fb = field_bytes(p, batch);
    unsigned char* base = (unsigned char*)ws;
    auto at = [&](int i) { return (cx<T>*)(base + (size_t)i * fb); };
    VjpWs<T> w;
    w.ubar = at(0);
    w.F = at(2);
    w.hf[0] = w.gm = at(6);
    w.hf[1] = w.hbar = at(7);
    w.X = at(8);
    w.ustart = at(12);
    w.u = at(13);
    w.stride = fb / sizeof(cx<T>);
    return w;
}

// Scratch of the adjoint model for a BUNDLE of K cotangents per trajectory (tcfd_ns2d_*_vjp_bundle): chunk-sized fields.  The
// first 8 are `Ws` again (the recomputation runs explicit_impl on them; its planes then hold the state's planes of the reversed
// stage), then the recomputed stage states, then what ONE GROUP of kg <= K cotangents needs in the sweep (nbar, the four Y planes,
// the four X spectra), then what every cotangent carries from stage to stage: 7 + nstages + 9 kg + 4 K fields.
// Y is stored [plane][cotangent][field] (`yplane_stride` per plane, `stride` per cotangent) and X likewise in the caller's pitch
// (`xplane_stride` per plane, `tan_stride` per cotangent), so that ONE column launch over kg * batch fields fills nbar or drains a
// plane of the group.  ubar, gm, hbar and ustart hold K cotangents of batch fields in the caller's pitch, `tan_stride` apart.
static inline int cobundle_fields(int ncot, int kg, int nstages) { return 7 + nstages + 9 * kg + 4 * ncot; }
template <typename T>
struct CoBundleWs {
    cx<T>* planes;        // Ws::planes: the state's four planes (plane 0 is F(u_k) while the stage states are recomputed)
    cx<T>* hf[2];         // Ws::upad, Ws::upad2: the accumulator h of the recomputation
    cx<T>* u;             // u_1 .. u_{nstages-1}, `stride` apart
    cx<T>* nbar;          // kg: the column-transformed gm of the group
    cx<T>* Y;             // 4 kg
    cx<T>* X;             // 4 kg
    cx<T>* ubar;          // K: the running cotangents of the state
    cx<T>* gm;            // K: the pre-weighted cotangents of F
    cx<T>* hbar;          // K: the cotangents of h
    cx<T>* ustart;        // K: the cotangents of the step's initial state through the base0 stages
    size_t stride;        // elements of one chunk-sized field
    size_t yplane_stride; // kg * stride
    size_t tan_stride;    // batch * n * m
    size_t xplane_stride; // kg * tan_stride
};
template <typename T>
static CoBundleWs<T> carve_cobundle(const tcfd_ns2d_plan* p, void* ws, long batch, int ncot, int kg, int nstages) {
    const size_t fb = field_bytes(p, batch);
    unsigned char* base = (unsigned char*)ws;
    auto at = [&](long i) { return (cx<T>*)(base + (size_t)i * fb); };
    CoBundleWs<T> w;
    w.planes = at(2);
    w.hf[0] = at(6);
    w.hf[1] = at(7);
    long i = 8;
    w.u = at(i); i += nstages - 1;
    w.nbar = at(i); i += kg;
    w.Y = at(i); i += 4L * kg;
    w.X = at(i); i += 4L * kg;
    w.ubar = at(i); i += ncot;
    w.gm = at(i); i += ncot;
    w.hbar = at(i); i += ncot;
    w.ustart = at(i);
    w.stride = fb / sizeof(cx<T>);
    w.yplane_stride = (size_t)kg * w.stride;
    w.tan_stride = (size_t)batch * p->n * p->m;
    w.xplane_stride = (size_t)kg * w.tan_stride;
    return w;
}

// One stage of the schedule with constant coefficients, written exactly as the fused forward kernels write it (k_cols, MODE_C):
//     h = fa f + beta h_prev ,    u = (b + gdt h + mu L b) / (1 - mud L)            (L: the real (n, m) linear term)
// Launched by tcfd_ns2d_stage_update (the differentiable step of autograd.py) and by the recomputation of tcfd_ns2d_step_vjp.
template <typename T>
__global__ __launch_bounds__(256) void k_stage_update(const cx<T>* __restrict__ f, const cx<T>* __restrict__ hp,
                                                      const cx<T>* __restrict__ b, const T* __restrict__ Lt, T fa, T beta, T gdt,
                                                      T mu, T mud, cx<T>* __restrict__ h, cx<T>* __restrict__ u, long total,
                                                      long plane) {
    using namespace tcfd;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const T L = Lt[e % plane];
        cx<T> hn = cscale(f[e], fa);
        if (hp) hn = hn + cscale(hp[e], beta);
        const cx<T> bv = b[e];
        const cx<T> rhs = bv + cscale(hn, gdt) + cscale(cscale(bv, L), mu);
        h[e] = hn;
        u[e] = cscale(rhs, fast_rcp((T)1 - mud * L));
    }
}

// Largest batch of one call: the launch grids and the block -> tile maps of the column kernels (ColArgs::batch, ntiles) are
// 32-bit.  A column grid is at most 2 (parities) x (batch x tiles rounded up to 8 line groups) <= batch (2 m + 16) workgroups
// with one-column tiles, a row grid batch n / 2: batch (n + 18) < 2^31 keeps every one of them, and every product of two of
// those ints, in range (n = 4096: 521 997 fields -- 70 TB of fp64 state, so memory ends a batch long before; element and byte
// offsets are size_t / long throughout).  Larger batches are refused, never wrapped.
static long max_batch(const tcfd_ns2d_plan* p) { return 2147483647L / (p->n + 18); }
static int check_batch(const tcfd_ns2d_plan* p, long batch) {
    if (batch > max_batch(p))
        return fail(TCFD_EINVAL, "batch %ld exceeds the largest batch of one call at n = %d (%ld fields)", batch, p->n, max_batch(p));
    return 0;
}
static int check_ws(const tcfd_ns2d_plan* p, long batch, void* ws, size_t bytes, size_t need) {
    if (int rc = check_batch(p, batch)) return rc;
    if (!ws || bytes < need) return fail(TCFD_EWORKSPACE, "workspace %zu B < required %zu B", bytes, need);
    return 0;
}

// ------------------------------------------------------------------ the sized units
// One function template per operation, on the real type only: tcfd_ns2d_sized.hip defines them (a switch over p->n into the
// size-templated drivers) and instantiates them for the type it is built for.  Arguments are checked and batches chunked by the
// callers in tcfd_ns2d.hip.
namespace ns2d {
template <typename T> int fill_round_fields(tcfd_ns2d_plan* p);
template <typename T>
int step(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch, int nstages, const double* beta,
         const double* gdt, const double* mu_num, const double* fa, const double* mu_den, const int* base0, int steps,
         double inv_total_dt, void* ws, hipStream_t st, long ens_b0);
// ens_b0: position of the chunk's first field in the caller's batch (the row of an ensemble plan's table it steps with)
template <typename T>
int explicit_terms(const tcfd_ns2d_plan* p, const void* w, void* out, const void* wt, void* psi, bool residual, long batch,
                   void* ws, hipStream_t st, long ens_b0);
template <typename T>
int explicit_vjp(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t x_field_stride, long batch, void* ws,
                 hipStream_t st);
template <typename T>
int explicit_jvp(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df, long batch, void* ws,
                 hipStream_t st);
template <typename T>
int step_jvp(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out, long batch, int nstages,
             const double* fa, const double* beta, const double* gdt, const double* mu_num, const double* mu_den,
             const int* base0, int steps, void* ws, hipStream_t st);
// one chunk of the tangent-bundle calls: ntan tangents per state, kg of them per pass through the sweep; tan_stride: elements
// between two tangents of the caller's arrays (the whole call's batch * n * m)
template <typename T>
int explicit_jvp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df, size_t tan_stride,
                        long batch, int ntan, int kg, void* ws, hipStream_t st);
template <typename T>
int step_jvp_bundle(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out, size_t tan_stride,
                    long batch, int ntan, int kg, int nstages, const double* fa, const double* beta, const double* gdt,
                    const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws, hipStream_t st);
// one chunk of tcfd_ns2d_step_vjp; saved_step_stride: elements between the saved inputs of two consecutive steps
template <typename T>
int step_vjp(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out, const void* pre,
             const void* post, void* g_in, long batch, int nstages, const double* fa, const double* beta, const double* gdt,
             const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws, hipStream_t st);
// one chunk of the cotangent-bundle calls: ncot cotangents per trajectory, kg of them per pass through the sweep; cot_stride:
// elements between two cotangents of the caller's arrays (the whole call's batch * n * m); xout: plane f of cotangent k is
// (4 k + f) cot_stride elements in
template <typename T>
int explicit_vjp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t cot_stride, long batch, int ncot,
                        int kg, void* ws, hipStream_t st);
template <typename T>
int step_vjp_bundle(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out, const void* pre,
                    const void* post, void* g_in, size_t cot_stride, long batch, int ncot, int kg, int nstages, const double* fa,
                    const double* beta, const double* gdt, const double* mu_num, const double* mu_den, const int* base0, int steps,
                    void* ws, hipStream_t st);
template <typename T> int rfft2(const tcfd_ns2d_plan* p, const void* x, void* out, long batch, hipStream_t st);
template <typename T> int irfft2(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, void* ws, hipStream_t st);
template <typename T> int irfft2_sub_max(const tcfd_ns2d_plan* p);
template <typename T>
int irfft2_sub(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, int S, void* ws, hipStream_t st);
template <typename T> int variant(const tcfd_ns2d_plan* p, int* split, int* rows_kernel);

// F(w) / residual sweep of a whole batch, chunk by chunk (tcfd_ns2d.hip; the refiner runs it on its own scratch)
int explicit_chunked(const tcfd_ns2d_plan* p, const void* w, void* out, const void* wt, void* psi, bool residual, long batch,
                     void* ws, hipStream_t st);
}  // namespace ns2d
