// capi.hip -- the contexts and everything of the C ABI / C++ API of libexblas.so (include/exblas_hip.h) that runs on one:
//   1. context lifecycle: the static per-device contexts (layer 0 for the device-pointer entries, layers 1.. for the
//      host-pointer layer), caller-owned handles, staging buffers and the workspace, the knobs and the last_*_info queries;
//   2. one implementation per routine on an explicit context (the *_on functions: argument checks, the context's lock,
//      the dispatch of blas1.hip ... bdot.hip);
//   3. the device-pointer ABI: exblas_X_ctx(handle, ...) resolves the handle (NULL: the device's default context) and
//      calls X_on; exblas_X_dev(...) is exblas_X_ctx(NULL, ...);
//   4. the host-pointer layer: ExSUM / ExDOT spread over the GPUs of the node (host_reduce), every other routine staged
//      through one private context (HostCall: copy in, one X_on call, copy out);
//   5. the C++ functions exsum/exdot/exgemv/extrsv/exgemm with the exact signatures of the reference's public headers
//      (include/blas1.hpp:48,74; blas2.hpp:57,95; blas3.hpp:56), which replace src/gpu/blas/blas{1,2,3}/Ex*.cpp: same
//      argument meaning, same variant dispatch, same error behaviour (print + exit on fpe < 0 or device failure, 0.0
//      for Ng <= 0 / unsupported variants).
// The generator and the bandwidth probes are in probes.hip, the multi-rank forms in comm.hip.
#include "../../include/exblas_hip.h"
#include "../../include/blas1.hpp"
#include "../../include/blas2.hpp"
#include "../../include/blas3.hpp"
#include "exblas_internal.h"
#include "superacc.hip.h"
#include "round_lowp.hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace exb {

static_assert(OUT_WORDS == EXBLAS_OUT_WORDS && OUT_CANON == EXBLAS_OUT_CANON && OUT_DIGITS == EXBLAS_OUT_DIGITS &&
                  NL == EXBLAS_NDIGITS && SET_WORDS == EXBLAS_SET_WORDS && CANON == EXBLAS_NCANON && OUT_EXACT == EXBLAS_OUT_EXACT &&
                  OUT_REFMODE == EXBLAS_OUT_REFMODE && OUT_FLAGS == EXBLAS_OUT_FLAGS,
              "record layout out of sync with include/exblas_hip.h");

[[noreturn]] void die(const char *what, hipError_t e, const char *file, int line)
{
    // the reference prints and exit(EXIT_FAILURE)s on any backend failure (gpu:ExSUM.cpp:111-115)
    fprintf(stderr, "exblas(hip): %s failed: %s (%s:%d)\n", what, hipGetErrorString(e), file, line);
    exit(EXIT_FAILURE);
}

static int env_int(const char *name, int dflt)
{
    const char *s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}

std::atomic<bool> g_comm_created{false};  // set by comm.hip when a communicator of more than one rank is created

static int g_round_mode = -1;
int round_mode()
{
    if (g_round_mode < 0) {
        const char *s = getenv("EXBLAS_ROUND");
        g_round_mode = (s && (s[0] == 'r' || s[0] == 'R' || s[0] == '1')) ? 1 : 0;
    }
    return g_round_mode;
}

static constexpr int MAX_DEV = 16;
static Ctx g_ctx[MAX_LAYERS][MAX_DEV];
static std::mutex g_ctx_mu;
static int g_last_layer[MAX_DEV];  // which layer ran the most recent exgemv / exgemm / extrsv (diagnostics only)

static int current_device()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d < MAX_DEV ? d : 0;
}

// (re)allocates the two accumulator sets of a context for its c.ngroups, zeroed; the caller has set the device
static void alloc_accumulators(Ctx &c)
{
    if (c.gacc_all) EXB_CHECK(hipFree(c.gacc_all));
    EXB_CHECK(hipMalloc(&c.gacc_all, 2 * sizeof(long long) * NL * c.ngroups));
    EXB_CHECK(hipMemset(c.gacc_all, 0, 2 * sizeof(long long) * NL * c.ngroups));
    c.gacc = c.gacc_all + (size_t)c.slot * NL * c.ngroups;
}

// creates the device objects of a context (accumulators, flags, record buffers, stream) on `device`; knobs come from the
// environment, then from the device's layer-0 context when that exists (what the API has set so far)
static void init_ctx(Ctx &c, int device, int layer)
{
    c.layer = layer;
    int prev = 0;
    EXB_CHECK(hipGetDevice(&prev));
    EXB_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    EXB_CHECK(hipGetDeviceProperties(&prop, device));
    c.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c.blocks_per_cu = env_int("EXBLAS_BLOCKS_PER_CU", 8);
    c.bpc_sum = env_int("EXBLAS_BPC_SUM", 2);
    c.bpc_dot = env_int("EXBLAS_BPC_DOT", 48);
    c.bpc_sa = env_int("EXBLAS_BPC_SA", 3);
    c.bpc_heavy = env_int("EXBLAS_BPC_HEAVY", 4);
    c.bpc_lp_sum = env_int("EXBLAS_BPC_LP_SUM", c.bpc_lp_sum);
    c.bpc_lp_dot = env_int("EXBLAS_BPC_LP_DOT", c.bpc_lp_dot);
    c.ngroups = env_int("EXBLAS_NGROUPS", 32);
    c.grid_adj = env_int("EXBLAS_GRID_ADJ", 0);
    if (c.ngroups < 1) c.ngroups = 1;
    c.gemm_path = env_int("EXBLAS_GEMM_PATH", 0);
    // knobs set through the API so far apply to every layer
    if (layer > 0 && g_ctx[0][device].device >= 0) static_cast<CtxKnobs &>(c) = g_ctx[0][device];
    EXB_CHECK(crt_tables_upload());
    c.slot = 0;
    alloc_accumulators(c);
    // per slot: the flag word (own 64-byte line) + the low and high accumulators of ExDOT (superacc.hip.h: low_acc_of, high_acc_of)
    EXB_CHECK(hipMalloc(&c.gflags_all, 2 * FLAG_BLOCK_BYTES));
    EXB_CHECK(hipMemset(c.gflags_all, 0, 2 * FLAG_BLOCK_BYTES));
    c.gflags = c.gflags_all;
    EXB_CHECK(hipMalloc(&c.d_record, sizeof(long long) * OUT_WORDS));
    // portable: the record of one device's part is copied to the first device when a host call spans several
    EXB_CHECK(hipHostMalloc(&c.h_record, sizeof(long long) * OUT_WORDS, hipHostMallocPortable));
    EXB_CHECK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    EXB_CHECK(hipDeviceSynchronize());
    EXB_CHECK(hipSetDevice(prev));
    c.device = device;
}

Ctx &ctx(int device, int layer)
{
    if (device < 0) {
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) {
            // no usable HIP device: the product path refuses to run (there is no CPU fallback)
            fprintf(stderr, "exblas(hip): no HIP device available: %s\n", hipGetErrorString(e));
            exit(EXIT_FAILURE);
        }
    }
    if (device >= MAX_DEV) {
        fprintf(stderr, "exblas(hip): device index %d out of range\n", device);
        exit(EXIT_FAILURE);
    }
    if (layer < 0 || layer >= MAX_LAYERS) layer = 0;
    Ctx &c = g_ctx[layer][device];
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (c.device < 0) init_ctx(c, device, layer);
    return c;
}

Ctx &default_ctx() { return ctx(-1); }

// run f on every context of the current device that exists (layer 0 is created if need be), each under its lock:
// tuning knobs and the workspace release are per device, not per layer
template <class F>
static void for_each_layer(F &&f)
{
    ctx(-1);
    const int device = current_device();
    for (int l = 0; l < MAX_LAYERS; ++l) {
        Ctx &c = g_ctx[l][device];
        if (c.device < 0) continue;
        std::lock_guard<std::mutex> lk(c.mu);
        f(c);
    }
}

void *stage_buf(Ctx &c, int slot, size_t bytes)
{
    if (bytes > c.stage_bytes[slot]) {
        if (c.stage[slot]) EXB_CHECK(hipFree(c.stage[slot]));
        size_t cap = bytes + (bytes >> 3) + 4096;
        EXB_CHECK(hipMalloc(&c.stage[slot], cap));
        c.stage_bytes[slot] = cap;
    }
    return c.stage[slot];
}

void *workspace(Ctx &c, size_t bytes, hipStream_t st, hipError_t *err)
{
    *err = hipSuccess;
    if (bytes > c.ws_bytes) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            // hipMalloc is illegal during capture, and the graph would bake in a pointer that the next growth moves
            *err = hipErrorStreamCaptureUnsupported;
            return nullptr;
        }
        // Allocate FIRST: only a successful growth may change the context.  On failure ws / ws_bytes / retired stay as
        // they were (the live block must never also sit in `retired`: a later exblas_release_retired_workspaces()
        // would free memory the next call launches into) and the failed hipMalloc's error is cleared, so that the
        // fallback path's hipGetLastError() does not report it.
        size_t cap = bytes + (c.ws_bytes >> 1);  // geometric growth bounds what the parked blocks can add up to
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, cap);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            cap = bytes;
            e = hipMalloc(&p, cap);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *err = e;
            return nullptr;
        }
        // the old block is parked, not freed: a graph captured earlier may still replay into it
        if (c.ws) c.retired.push_back(c.ws);
        c.ws = p;
        c.ws_bytes = cap;
    }
    return c.ws;
}

}  // namespace exb

using namespace exb;

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int exblas_hip_init(int device)
{
    ctx(device);
    return 0;
}

int exblas_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *exblas_hip_version(void) { return "exblas-hip 0.1 (gfx950)"; }

void exblas_set_round_mode(int mode) { g_round_mode = mode ? 1 : 0; }

int exblas_set_tuning(int blocks_per_cu, int ngroups, int variant)
{
    // variant: kept in the signature for existing callers.  Refused before the device is touched: a stale A/B script
    // fails instead of timing the one production kernel under a variant's name.
    if (variant != -1 && variant != 0) return (int)hipErrorInvalidValue;
    for_each_layer([&](Ctx &c) {
        if (blocks_per_cu > 0) c.blocks_per_cu = c.bpc_sum = c.bpc_dot = c.bpc_sa = c.bpc_heavy = c.bpc_lp_sum = c.bpc_lp_dot = blocks_per_cu;
        if (ngroups > 0 && ngroups != c.ngroups) {
            EXB_CHECK(hipDeviceSynchronize());
            c.ngroups = ngroups;
            alloc_accumulators(c);
            EXB_CHECK(hipDeviceSynchronize());
        }
    });
    return 0;
}
int exblas_get_round_mode(void) { return round_mode(); }

int exblas_set_accumulator_slot(int slot)
{
    Ctx &c = ctx(-1);
    std::lock_guard<std::mutex> lk(c.mu);
    if (slot < 0 || slot > 1) return (int)hipErrorInvalidValue;
    c.slot = slot;
    c.gacc = c.gacc_all + (size_t)slot * NL * c.ngroups;
    c.gflags = (unsigned *)((char *)c.gflags_all + (size_t)FLAG_BLOCK_BYTES * slot);
    return 0;
}

int exblas_set_launch_events(void *ev_start, void *ev_stop)
{
    Ctx &c = ctx(-1);
    std::lock_guard<std::mutex> lk(c.mu);
    c.launch_start_event = (hipEvent_t)ev_start;
    c.launch_stop_event = (hipEvent_t)ev_stop;
    return 0;
}

// out[0] = implementation of the most recent exgemm on this device (0 scalar kernel, 1 fp64 slices on MFMA-F64,
// 2 int8 digit slices, 4 int8 residues).  Slices: out[1] / out[2] = slices of A / B.  Residues: out[1] / out[2] = bits
// of the fixed-point entries of A' / B, out[3] = moduli, out[4] = moduli the workspace was reserved for.  The rest 0.
// The int8 paths decide on the device: this call then synchronises the device and reads the decision back.
static int last_gemm_info_on(Ctx &c, int *out)
{
    std::lock_guard<std::mutex> lk(c.mu);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (c.gemm_info_dev) {
        int h[INFO_WORDS];
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        if (hipMemcpy(h, c.gemm_info_dev, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        out[0] = (h[INFO_PATH] == PATH_I8 || h[INFO_PATH] == PATH_CRT) ? h[INFO_PATH] : PATH_SCALAR;
        if (out[0] == PATH_I8) {
            out[1] = h[INFO_SA];
            out[2] = h[INFO_SB];
        } else if (out[0] == PATH_CRT) {
            out[1] = h[INFO_CRT_NA];
            out[2] = h[INFO_CRT_NB];
            out[3] = h[INFO_CRT_L];     // moduli = int8 GEMMs
            out[4] = c.gemm_ws_moduli;  // 39 unless memory ran short
        }
    } else if (c.last_gemm_slices > 0) {
        out[0] = 1;
        out[1] = out[2] = c.last_gemm_slices;
    }
    return 0;
}

int exblas_last_gemm_info(int *out) { return last_gemm_info_on(ctx(-1, g_last_layer[current_device()]), out); }

int exblas_last_gemm_slices(void)
{
    int v[8];
    if (exblas_last_gemm_info(v) != 0) return -1;
    if (v[0] == 4) return v[3];  // residue path: the number of moduli (= int8 GEMMs)
    return v[1] > v[2] ? v[1] : v[2];
}

// The last streaming ExSUM / ExDOT launch of the current device's default context (the *_dev entry points): out[0] the
// kernel (1 fp64 ExSUM on k_blas1_stream, 2 on k_blas1_strided, 3 and 4 fp64 ExDOT likewise, 5 .. 8 the same of blas1_lowp.hip; 0: none yet), out[1] its grid, out[2] the group
// accumulators, out[3] the compute units the geometry was sized for, out[4..7] reserved.  Host state only: nothing is
// read from the device and nothing synchronises.
int exblas_last_blas1_info(int *out)
{
    if (!out) return (int)hipErrorInvalidValue;
    Ctx &c = ctx(-1);
    std::lock_guard<std::mutex> lk(c.mu);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = c.last_blas1_kernel;
    out[1] = c.last_blas1_grid;
    out[2] = c.ngroups;
    out[3] = c.num_cu;
    return 0;
}

void exblas_set_gemm_max_slices(int s) { for_each_layer([&](Ctx &c) { c.gemm_max_slices = s; }); }
void exblas_set_gemm_max_moduli(int l) { for_each_layer([&](Ctx &c) { c.gemm_max_moduli = l; }); }
void exblas_set_gemm_path(int mode) { for_each_layer([&](Ctx &c) { c.gemm_path = mode; }); }

// a path knob of every context of the device: `mode` in [0, largest], anything else means 0 (automatic)
static void set_path(int CtxKnobs::*knob, int mode, int largest)
{
    for_each_layer([&](Ctx &c) { c.*knob = (mode >= 0 && mode <= largest) ? mode : 0; });
}
void exblas_set_spmv_path(int mode) { set_path(&CtxKnobs::spmv_path, mode, 3); }
void exblas_set_spmm_path(int mode) { set_path(&CtxKnobs::spmm_path, mode, 3); }
void exblas_set_sptrsv_path(int mode) { set_path(&CtxKnobs::sptrsv_path, mode, 2); }
void exblas_set_spilu0_path(int mode) { set_path(&CtxKnobs::spilu0_path, mode, 2); }
void exblas_set_spic0_path(int mode) { set_path(&CtxKnobs::spic0_path, mode, 2); }
void exblas_set_sptrsm_path(int mode) { set_path(&CtxKnobs::sptrsm_path, mode, 3); }
void exblas_set_trsm_path(int mode) { set_path(&CtxKnobs::trsm_path, mode, 3); }
void exblas_set_bdot_path(int mode) { set_path(&CtxKnobs::bdot_path, mode, 2); }
void exblas_set_bgemm_path(int mode) { set_path(&CtxKnobs::bgemm_path, mode, 3); }
void exblas_set_btrsm_path(int mode) { set_path(&CtxKnobs::btrsm_path, mode, 3); }
void exblas_set_potrf_path(int mode) { set_path(&CtxKnobs::potrf_path, mode, 3); }
void exblas_set_potrf_batched_path(int mode) { set_path(&CtxKnobs::potrf_batched_path, mode, 3); }
void exblas_set_potrs_batched_path(int mode) { set_path(&CtxKnobs::potrs_batched_path, mode, 3); }
void exblas_set_getrf_batched_path(int mode) { set_path(&CtxKnobs::getrf_batched_path, mode, 3); }
void exblas_set_getrs_batched_path(int mode) { set_path(&CtxKnobs::getrs_batched_path, mode, 3); }

// the 8-word workspace header of a context's last sparse call (zeros when it launched nothing, or on failure); synchronises
static int sparse_header(const long long *info_dev, long long (&h)[8])
{
    for (int i = 0; i < 8; ++i) h[i] = 0;
    if (!info_dev) return 0;
    if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, info_dev, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
        return 0;
    for (int i = 0; i < 8; ++i) h[i] = 0;
    return -1;
}

// what the last solve of a context (its lock held) has to report, h receiving its header: 0, EXBLAS_SPTRSV_STALLED when
// that call's watchdog was raised, or the error of reading the header
static int solve_status(const long long *info_dev, long long (&h)[8])
{
    if (int e = sparse_header(info_dev, h)) return e;
    return h[1] ? EXBLAS_SPTRSV_STALLED : 0;
}

// The four counters of the last sparse call on the last-used layer.  ExSpMV / ExSpMM: -1 when there was no call.  The two
// solves (`solve`): a call that launched nothing counts zeros; EXBLAS_SPTRSV_STALLED when that call's watchdog was raised.
static int last_sparse_info(const long long *CtxWsPtrs::*info_dev, bool solve, int64_t *out4)
{
    if (!out4) return (int)hipErrorInvalidValue;
    Ctx &c = ctx(-1, g_last_layer[current_device()]);
    std::lock_guard<std::mutex> lk(c.mu);
    long long h[8];
    const int rc = solve ? solve_status(c.*info_dev, h) : sparse_header(c.*info_dev, h);
    for (int i = 0; i < 4; ++i) out4[i] = h[4 + i];
    return (!solve && !(c.*info_dev)) ? -1 : rc;   // (rc: 0, -1 when the header could not be read, or the solve's status)
}

// out[0] rows rounded in registers, out[1] rows rounded from their accumulator, out[2] rows split across workgroups,
// out[3] chunks of the split rows
int exblas_last_spmv_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::spmv_info_dev, false, out4); }

// out[0] outputs rounded in registers, out[1] outputs rounded from an accumulator, out[2] rows split across workgroups,
// out[3] chunks of the split rows
int exblas_last_spmm_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::spmm_info_dev, false, out4); }

// out[0] rows rounded in registers, out[1] rows rounded from their accumulator, out[2] rows without a stored diagonal
// under 'N', out[3] stored entries skipped; EXBLAS_SPTRSV_STALLED when the watchdog of that call was raised
int exblas_last_sptrsv_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::sptrsv_info_dev, true, out4); }

// out[0] entries rounded in registers, out[1] entries rounded from the accumulator, out[2] product terms summed, out[3] rows
// in the several-entries-per-lane form; EXBLAS_SPTRSV_STALLED as above
int exblas_last_spilu0_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::spilu0_info_dev, true, out4); }

// out[0] entries rounded in registers, out[1] entries rounded from the accumulator (both on and below the diagonal only),
// out[2] product terms summed, out[3] rows in the several-entries-per-lane form; EXBLAS_SPTRSV_STALLED as above
int exblas_last_spic0_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::spic0_info_dev, true, out4); }

// out[0] outputs rounded in registers, out[1] outputs rounded from the accumulator, out[2] rows without a stored diagonal
// under 'N', out[3] stored entries skipped (the structure counts once, whatever k); EXBLAS_SPTRSV_STALLED as above
int exblas_last_sptrsm_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::sptrsm_info_dev, true, out4); }

// out[0] outputs rounded in registers, out[1] outputs rounded from the accumulator, out[2] = out[3] = 0 (a dense triangle
// has no structure to count); EXBLAS_SPTRSV_STALLED as above
int exblas_last_trsm_info(int64_t *out4) { return last_sparse_info(&CtxWsPtrs::trsm_info_dev, true, out4); }

// The counters of the last ExBGEMM / ExBTRSM on the last-used layer: the kernel leaves one pair per workgroup (nothing
// has to be zeroed before it runs), they are added up here.  All 0 after a call that launched nothing.  Synchronises.
static int last_slot_info(SlotInfo CtxWsPtrs::*slots, int64_t *out4)
{
    if (!out4) return (int)hipErrorInvalidValue;
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    Ctx &c = ctx(-1, g_last_layer[current_device()]);
    std::lock_guard<std::mutex> lk(c.mu);
    const SlotInfo &s = c.*slots;
    if (!s.dev || s.blocks <= 0) return 0;
    std::vector<long long> h((size_t)s.blocks * 2);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h.data(), s.dev, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (size_t b = 0; b < h.size(); b += 2) {
        out4[0] += h[b];
        out4[1] += h[b + 1];
    }
    return 0;
}

// out[0] outputs rounded in registers, out[1] outputs rounded from the accumulator, out[2] = out[3] = 0
int exblas_last_bgemm_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::bgemm_slots, out4); }

// the same for ExBTRSM
int exblas_last_btrsm_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::btrsm_slots, out4); }

// the same for ExPOTRF: out[0] + out[1] is the number of entries the call fixed (the radicand of a breakdown included)
int exblas_last_potrf_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::potrf_slots, out4); }

// the same for the batched ExPOTRF: out[0] + out[1] is the number of entries fixed over the whole batch
int exblas_last_potrf_batched_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::potrf_batched_slots, out4); }

// the same for the batched ExPOTRS: out[0] + out[1] is n * k per sweep
int exblas_last_potrs_batched_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::potrs_batched_slots, out4); }

// the same for the batched ExGETRF: out[0] + out[1] is the number of roundings over the whole batch (p^2 per complete matrix)
int exblas_last_getrf_batched_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::getrf_batched_slots, out4); }

// the same for the batched ExGETRS: out[0] + out[1] is 2 n k
int exblas_last_getrs_batched_info(int64_t *out4) { return last_slot_info(&CtxWsPtrs::getrs_batched_slots, out4); }

// ---- implementations on an explicit context (layer 0 for the *_dev entry points, a private one for host calls) ----
static int exsum_accumulate_on(Ctx &c, const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                               hipStream_t st)
{
    if (fpe < 0 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    // unsupported (fpe, early_exit) combination: nothing is launched, the accumulators stay zero -> 0.0
    return n > 0 ? (int)exsum_dispatch(c, d_a, n, inca, fpe, early_exit, st) : 0;
}

static int exdot_accumulate_on(Ctx &c, const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n,
                               int fpe, int early_exit, hipStream_t st)
{
    if (fpe < 0 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    return n > 0 ? (int)exdot_dispatch(c, d_a, inca, d_b, incb, n, fpe, early_exit, st) : 0;
}

static int finish_on(Ctx &c, hipStream_t st, int64_t *d_out)
{
    std::lock_guard<std::mutex> lk(c.mu);
    return (int)finalize_groups(c, st, (long long *)d_out);
}

// The narrow-input forms (blas1_lowp.hip).  What they refuse is decided from the arguments alone, before any context is
// looked up: 0, or hipErrorInvalidValue.  b == nullptr with incb == 1: ExSUM.
static int lp_refused(int dtype, const void *a, int64_t inca, const void *b, int64_t incb, int64_t n, int fpe)
{
    if (!dtype_known(dtype) || fpe < 0 || fpe > 8 || inca < 1 || incb < 1 || n < 0 || n > 0x7fffffffll)
        return (int)hipErrorInvalidValue;
    const uintptr_t mask = (uintptr_t)dtype_bytes(dtype) - 1;
    return (((uintptr_t)a | (uintptr_t)b) & mask) ? (int)hipErrorInvalidValue : 0;
}

static int exsum_lp_accumulate_on(Ctx &c, int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                                  hipStream_t st)
{
    if (int rc = lp_refused(dtype, d_a, inca, nullptr, 1, n, fpe)) return rc;
    if (dtype == DT_F64) return exsum_accumulate_on(c, (const double *)d_a, n, inca, fpe, early_exit, st);
    std::lock_guard<std::mutex> lk(c.mu);
    return n > 0 ? (int)exsum_lp_dispatch(c, dtype, d_a, n, inca, fpe, st) : 0;
}

static int exdot_lp_accumulate_on(Ctx &c, int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb,
                                  int64_t n, int fpe, int early_exit, hipStream_t st)
{
    if (int rc = lp_refused(dtype, d_a, inca, d_b, incb, n, fpe)) return rc;
    if (dtype == DT_F64)
        return exdot_accumulate_on(c, (const double *)d_a, inca, (const double *)d_b, incb, n, fpe, early_exit, st);
    std::lock_guard<std::mutex> lk(c.mu);
    return n > 0 ? (int)exdot_lp_dispatch(c, dtype, d_a, inca, d_b, incb, n, fpe, st) : 0;
}

static int round_records_refused(const int64_t *d_records, int64_t count, int64_t stride_words, int dtype, const void *d_out)
{
    const bool bad = !dtype_known(dtype) || count < 0 || (count > 1 && stride_words < OUT_WORDS) ||
                     (count > 0 && (!d_records || !d_out));
    return bad ? (int)hipErrorInvalidValue : 0;
}

static int exgemv_on(Ctx &c, char transa, int m, int n, double alpha, const double *d_a, int lda, const double *d_x,
                     int incx, double beta, double *d_y, int incy, int fpe, int early_exit, hipStream_t st)
{
    if (fpe < 0) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exgemv_dispatch(c, transa, m, n, alpha, d_a, lda, d_x, incx, beta, d_y, incy, fpe, early_exit,
                                round_mode(), st);
}

// The argument checks of the CSR calls, on host or device pointers alike (ExSpMV: k = 1, ldx = ldy = 1).  *empty: nothing
// to compute (m == 0 or k == 0), which is decided before the pointers are looked at.
static int csr_check_args(int m, int n, int k, int index_bits, const void *row_ptr, const double *x, int64_t ldx,
                          const double *y, int64_t ldy, int fpe, bool *empty)
{
    *empty = false;
    if (m < 0 || n < 0 || k < 0 || fpe < 0 || (index_bits != 32 && index_bits != 64)) return (int)hipErrorInvalidValue;
    if (ldx < k || ldy < k) return (int)hipErrorInvalidValue;
    *empty = m == 0 || k == 0;
    if (!*empty && (!row_ptr || !y || (n > 0 && !x))) return (int)hipErrorInvalidValue;
    return 0;
}

static int exspmv_on(Ctx &c, int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                     const double *d_val, double alpha, const double *d_x, double beta, double *d_y, int fpe,
                     int early_exit, hipStream_t st)
{
    bool empty;   // m == 0 goes on: the call still counts as the device's last one, and the dispatch launches nothing
    if (int rc = csr_check_args(m, n, 1, index_bits, d_row_ptr, d_x, 1, d_y, 1, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspmv_dispatch(c, m, n, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, beta, d_y, fpe,
                                early_exit, round_mode(), st);
}

static int exspmm_on(Ctx &c, int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                     const double *d_val, double alpha, const double *d_x, int64_t ldx, double beta, double *d_y,
                     int64_t ldy, int fpe, int early_exit, hipStream_t st)
{
    bool empty;
    const int rc = csr_check_args(m, n, k, index_bits, d_row_ptr, d_x, ldx, d_y, ldy, fpe, &empty);
    if (rc || empty) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspmm_dispatch(c, m, n, k, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, ldx, beta, d_y, ldy,
                                fpe, early_exit, round_mode(), st);
}

// The narrow CSR entries: what they refuse beyond csr_check_args, before a device is needed.  The pair (float64, float64)
// is the fp64 entry's business (*forward); fpe = 1 has no narrow kernel.
static int csr_lp_refused(int val_dtype, const void *val, int vec_dtype, const void *x, const void *y, int fpe, bool *forward)
{
    *forward = false;
    if (!dtype_known(val_dtype) || !dtype_known(vec_dtype)) return (int)hipErrorInvalidValue;
    if (vec_dtype != DT_F64 && vec_dtype != val_dtype) return (int)hipErrorInvalidValue;
    const uintptr_t vmask = (uintptr_t)dtype_bytes(val_dtype) - 1, xmask = (uintptr_t)dtype_bytes(vec_dtype) - 1;
    if (((uintptr_t)val & vmask) || ((uintptr_t)x & xmask) || ((uintptr_t)y & xmask)) return (int)hipErrorInvalidValue;
    *forward = val_dtype == DT_F64;
    if (*forward) return 0;
    if (fpe < 0 || fpe > 8) return (int)hipErrorInvalidValue;
    return fpe == 1 ? EXBLAS_UNSUPPORTED : 0;
}

static int exspmv_lp_on(Ctx &c, int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx, int val_dtype,
                        const void *d_val, double alpha, int vec_dtype, const void *d_x, double beta, void *d_y, int fpe,
                        int early_exit, hipStream_t st)
{
    bool forward, empty;
    if (int rc = csr_lp_refused(val_dtype, d_val, vec_dtype, d_x, d_y, fpe, &forward)) return rc;
    if (forward)
        return exspmv_on(c, m, n, index_bits, d_row_ptr, d_col_idx, (const double *)d_val, alpha, (const double *)d_x, beta,
                         (double *)d_y, fpe, early_exit, st);
    if (int rc = csr_check_args(m, n, 1, index_bits, d_row_ptr, (const double *)d_x, 1, (const double *)d_y, 1, fpe, &empty))
        return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspmv_lp_dispatch(c, m, n, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype, d_x, beta,
                                   d_y, fpe, round_mode(), st);
}

static int exspmm_lp_on(Ctx &c, int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                        int val_dtype, const void *d_val, double alpha, int vec_dtype, const void *d_x, int64_t ldx,
                        double beta, void *d_y, int64_t ldy, int fpe, int early_exit, hipStream_t st)
{
    bool forward, empty;
    if (int rc = csr_lp_refused(val_dtype, d_val, vec_dtype, d_x, d_y, fpe, &forward)) return rc;
    if (forward)
        return exspmm_on(c, m, n, k, index_bits, d_row_ptr, d_col_idx, (const double *)d_val, alpha, (const double *)d_x,
                         ldx, beta, (double *)d_y, ldy, fpe, early_exit, st);
    const int rc = csr_check_args(m, n, k, index_bits, d_row_ptr, (const double *)d_x, ldx, (const double *)d_y, ldy, fpe,
                                  &empty);
    if (rc || empty) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspmm_lp_dispatch(c, m, n, k, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype, d_x,
                                   ldx, beta, d_y, ldy, fpe, round_mode(), st);
}

// what the narrow CSR entries refuse without a context: csr_lp_refused, then (unless the fp64 entry takes over) the shape
// rules of csr_check_args
static int csr_lp_precheck(int m, int n, int k, int index_bits, const void *row_ptr, int val_dtype, const void *val,
                           int vec_dtype, const void *x, int64_t ldx, const void *y, int64_t ldy, int fpe)
{
    bool forward, empty;
    if (int rc = csr_lp_refused(val_dtype, val, vec_dtype, x, y, fpe, &forward)) return rc;
    return csr_check_args(m, n, k, index_bits, row_ptr, (const double *)x, ldx, (const double *)y, ldy, fpe, &empty);
}

static bool one_of(char ch, const char *set) { return ch != 0 && strchr(set, ch) != nullptr; }

// The argument checks of ExBDOT, on host or device pointers alike.  *empty: nothing to compute (p == 0 or q == 0), which
// is decided before the pointers are looked at.
static int bdot_check_args(char mode, int64_t n, int p, int q, const double *x, int64_t ldx, const double *y, int64_t ldy,
                           const double *c, int64_t ldc, int fpe, bool *empty)
{
    *empty = false;
    if (!one_of(mode, "GgDd") || n < 0 || n > 0x7fffffffll || p < 0 || q < 0 || fpe < 0) return (int)hipErrorInvalidValue;
    const bool diag = mode == 'D' || mode == 'd';
    if (ldx < p || ldy < q || (diag ? p != q : ldc < q)) return (int)hipErrorInvalidValue;
    *empty = p == 0 || q == 0;
    if (!*empty && (!c || (n > 0 && (!x || !y)))) return (int)hipErrorInvalidValue;
    return 0;
}

// (the arguments of the two below were checked by their callers, before those needed a context)
static int exbdot_on(Ctx &c, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y,
                     int64_t ldy, double *d_c, int64_t ldc, int fpe, int early_exit, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(c.mu);
    return (int)exbdot_dispatch(c, mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, early_exit, round_mode(), st);
}

// The row-sharded forms of ExBDOT.  Export: bdot_check_args' rules with the sets in C's place, and the two combinations
// that have no digit sets to give -- plain fp64 sums (fpe == 1) and the silent return (early exit with fpe > 8), which
// would leave the caller's sets undefined.
static int bdot_export_check(char mode, int64_t n, int p, int q, const double *x, int64_t ldx, const double *y, int64_t ldy,
                             const int64_t *sets, int fpe, int early_exit, bool *empty)
{
    const int rc = bdot_check_args(mode, n, p, q, x, ldx, y, ldy, (const double *)sets, q, fpe, empty);
    if (rc) return rc;
    return (fpe == 1 || (early_exit && fpe > 8)) ? (int)hipErrorInvalidValue : 0;
}

static int exbdot_export_on(Ctx &c, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y,
                            int64_t ldy, int64_t *d_sets, int fpe, int early_exit, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(c.mu);
    return exbdot_export_dispatch(c, mode, n, p, q, d_x, ldx, d_y, ldy, (long long *)d_sets, fpe, early_exit, st);
}

static int bdot_round_check(char mode, int p, int q, const int64_t *sets, int nsets, const double *c, int64_t ldc, bool *empty)
{
    *empty = false;
    if (!one_of(mode, "GgDd") || p < 0 || q < 0 || nsets < 1) return (int)hipErrorInvalidValue;
    const bool diag = mode == 'D' || mode == 'd';
    if (diag ? p != q : ldc < q) return (int)hipErrorInvalidValue;
    *empty = p == 0 || q == 0;
    if (!*empty && (!c || !sets)) return (int)hipErrorInvalidValue;
    return 0;
}

static int exsptrsv_on(Ctx &c, char uplo, char diag, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                       const double *d_val, double *d_x, int fpe, int early_exit, hipStream_t st)
{
    if (!one_of(uplo, "LlUu") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    bool empty;   // m == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = csr_check_args(m, 0, 1, index_bits, d_row_ptr, nullptr, 1, d_x, 1, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exsptrsv_dispatch(c, uplo, diag, m, index_bits, d_row_ptr, d_col_idx, d_val, d_x, fpe, early_exit,
                                  round_mode(), st);
}

// m == 0 goes on: info is still zeroed, and the call counts as the device's last one
static int exspilu0_on(Ctx &c, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                       double *d_lu, int64_t *d_info, int fpe, int early_exit, hipStream_t st)
{
    if (m < 0 || fpe < 0 || (index_bits != 32 && index_bits != 64) || !d_info) return (int)hipErrorInvalidValue;
    if (m > 0 && !d_row_ptr) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspilu0_dispatch(c, m, index_bits, d_row_ptr, d_col_idx, d_val, d_lu, (long long *)d_info, fpe, early_exit,
                                  round_mode(), st);
}

// the checks of exspilu0_on, which need no context: the device entries make them before one is looked up
static bool spic0_args_bad(int m, int index_bits, const void *d_row_ptr, const int64_t *d_info, int fpe)
{
    return m < 0 || fpe < 0 || (index_bits != 32 && index_bits != 64) || !d_info || (m > 0 && !d_row_ptr);
}

static int exspic0_on(Ctx &c, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                      double *d_ll, int64_t *d_info, int fpe, int early_exit, hipStream_t st)
{
    if (spic0_args_bad(m, index_bits, d_row_ptr, d_info, fpe)) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exspic0_dispatch(c, m, index_bits, d_row_ptr, d_col_idx, d_val, d_ll, (long long *)d_info, fpe, early_exit,
                                 round_mode(), st);
}

static int exsptrsm_on(Ctx &c, char uplo, char diag, int m, int k, int index_bits, const void *d_row_ptr,
                       const void *d_col_idx, const double *d_val, double *d_x, int64_t ldx, int fpe, int early_exit,
                       hipStream_t st)
{
    if (!one_of(uplo, "LlUu") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    bool empty;   // m == 0 or k == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = csr_check_args(m, 0, k, index_bits, d_row_ptr, nullptr, k, d_x, ldx, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exsptrsm_dispatch(c, uplo, diag, m, k, index_bits, d_row_ptr, d_col_idx, d_val, d_x, ldx, fpe, early_exit,
                                  round_mode(), st);
}

static int extrsv_on(Ctx &c, char uplo, char transa, char diag, int n, const double *d_a, int lda, double *d_x,
                     int incx, int fpe, int early_exit, hipStream_t st)
{
    if (fpe < 0) return (int)hipErrorInvalidValue;
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    if (n > 0 && (lda < n || incx <= 0)) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)extrsv_dispatch(c, uplo, transa, diag, n, d_a, lda, d_x, incx, fpe, early_exit, round_mode(), st);
}

// The argument checks of ExTRSM, on host or device pointers alike; fpe >= 9 is refused as ExTRSV refuses it.  *empty:
// nothing to compute (n == 0 or k == 0), which is decided before the pointers are looked at.
static int trsm_check_args(char uplo, char transa, char diag, int n, int k, const double *a, int lda, const double *x,
                           int64_t ldx, int fpe, bool *empty)
{
    *empty = false;
    if (!one_of(uplo, "LlUu") || !one_of(transa, "NnTt") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    if (n < 0 || k < 0 || lda < (n > 1 ? n : 1) || ldx < k || fpe < 0) return (int)hipErrorInvalidValue;
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    *empty = n == 0 || k == 0;
    if (!*empty && (!a || !x)) return (int)hipErrorInvalidValue;
    return 0;
}

static int extrsm_on(Ctx &c, char uplo, char transa, char diag, int n, int k, const double *d_a, int lda, double *d_x,
                     int64_t ldx, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // n == 0 or k == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = trsm_check_args(uplo, transa, diag, n, k, d_a, lda, d_x, ldx, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)extrsm_dispatch(c, uplo, transa, diag, n, k, d_a, lda, d_x, ldx, fpe, early_exit, round_mode(), st);
}

// The argument checks of ExBGEMM, on host or device pointers alike.  *empty: nothing to compute (n == 0 or q == 0), which
// is decided before the pointers are looked at.
static int bgemm_check_args(int64_t n, int p, int q, const double *x, int64_t ldx, const double *cm, int64_t ldc,
                            const double *y, int64_t ldy, int fpe, bool *empty)
{
    *empty = false;
    if (n < 0 || n > 0x7fffffffll || p < 0 || q < 0 || fpe < 0) return (int)hipErrorInvalidValue;
    if (ldx < p || ldc < q || ldy < q) return (int)hipErrorInvalidValue;
    *empty = n == 0 || q == 0;
    if (!*empty && (!y || (p > 0 && (!x || !cm)))) return (int)hipErrorInvalidValue;
    return 0;
}

static int exbgemm_on(Ctx &c, int64_t n, int p, int q, double alpha, const double *d_x, int64_t ldx, const double *d_c,
                      int64_t ldc, double beta, double *d_y, int64_t ldy, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // n == 0 or q == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = bgemm_check_args(n, p, q, d_x, ldx, d_c, ldc, d_y, ldy, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exbgemm_dispatch(c, n, p, q, alpha, d_x, ldx, d_c, ldc, beta, d_y, ldy, fpe, early_exit, round_mode(), st);
}

// The argument checks of ExBTRSM, on host or device pointers alike, before a device is touched; fpe >= 9 is refused as
// ExTRSM refuses it.  *empty: nothing to compute (n == 0 or p == 0), which is decided before the pointers are looked at.
static int btrsm_check_args(char uplo, char transt, char diag, int64_t n, int p, const double *t, int ldt, const double *x,
                            int64_t ldx, int fpe, bool *empty)
{
    *empty = false;
    if (!one_of(uplo, "LlUu") || !one_of(transt, "NnTt") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    if (n < 0 || p < 0 || p > EXBLAS_BTRSM_MAX_P || ldt < (p > 1 ? p : 1) || ldx < p || fpe < 0)
        return (int)hipErrorInvalidValue;
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    *empty = n == 0 || p == 0;
    if (!*empty && (!t || !x)) return (int)hipErrorInvalidValue;
    return 0;
}

static int exbtrsm_on(Ctx &c, char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *d_t, int ldt,
                      double *d_x, int64_t ldx, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // n == 0 or p == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = btrsm_check_args(uplo, transt, diag, n, p, d_t, ldt, d_x, ldx, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exbtrsm_dispatch(c, uplo, transt, diag, n, p, alpha, d_t, ldt, d_x, ldx, fpe, early_exit, round_mode(), st);
}

// The argument checks of ExPOTRF, on host or device pointers alike, before a device is touched.  *empty: p == 0, which
// is decided before the pointers are looked at.
static int potrf_check_args(char uplo, int p, const double *g, int ldg, const int *info, int fpe, bool *empty)
{
    *empty = false;
    if (!one_of(uplo, "LlUu") || p < 0 || p > EXBLAS_BTRSM_MAX_P || ldg < (p > 1 ? p : 1) || fpe < 0)
        return (int)hipErrorInvalidValue;
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    *empty = p == 0;
    if (!*empty && (!g || !info)) return (int)hipErrorInvalidValue;
    return 0;
}

static int expotrf_on(Ctx &c, char uplo, int p, double *d_g, int ldg, int *d_info, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // p == 0 goes on: the call counts as the device's last one, and the dispatch launches nothing
    if (int rc = potrf_check_args(uplo, p, d_g, ldg, d_info, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)expotrf_dispatch(c, uplo, p, d_g, ldg, d_info, fpe, early_exit, round_mode(), st);
}

// The argument checks of the two batched factorisations (ExPOTRF: flag = uplo of "LlUu", ExGETRF: flag = order of "CcRr"),
// on host or device pointers alike, before a device is touched.  outs: the output pointers (info; ipiv and info) are all
// there.  *empty: p == 0 or batch == 0, which is decided before the pointers are looked at.
static int bjacobi_factor_check_args(char flag, const char *flags, int p, int max_p, int64_t batch, const double *a, int lda,
                                     int64_t stride, bool outs, int fpe, bool *empty)
{
    *empty = false;
    if (!one_of(flag, flags) || p < 0 || batch < 0 || p > max_p || lda < (p > 1 ? p : 1) || fpe < 0)
        return (int)hipErrorInvalidValue;
    if (batch > 1 && stride < (int64_t)lda * p) return (int)hipErrorInvalidValue;
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    *empty = p == 0 || batch == 0;
    if (!*empty && (!a || !outs)) return (int)hipErrorInvalidValue;
    return 0;
}

static int potrf_batched_check_args(char uplo, int p, int64_t batch, const double *g, int ldg, int64_t stride, const int *info,
                                    int fpe, bool *empty)
{
    return bjacobi_factor_check_args(uplo, "LlUu", p, EXBLAS_POTRF_BATCHED_MAX_P, batch, g, ldg, stride, info != nullptr, fpe,
                                     empty);
}

static int getrf_batched_check_args(char order, int p, int64_t batch, const double *a, int lda, int64_t stride, const int *ipiv,
                                    const int *info, int fpe, bool *empty)
{
    return bjacobi_factor_check_args(order, "CcRr", p, EXBLAS_GETRF_BATCHED_MAX_P, batch, a, lda, stride, ipiv && info, fpe,
                                     empty);
}

static int expotrf_batched_on(Ctx &c, char uplo, int p, int64_t batch, double *d_g, int ldg, int64_t stride, int *d_info,
                              int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // an empty call goes on: it counts as the device's last one, and the dispatch launches nothing
    if (int rc = potrf_batched_check_args(uplo, p, batch, d_g, ldg, stride, d_info, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)expotrf_batched_dispatch(c, uplo, p, batch, d_g, ldg, stride, d_info, fpe, early_exit, round_mode(), st);
}

// The argument checks of the two batched applies (ExPOTRS: flags_ok = uplo of "LlUu" and sweep of "12Bb", ExGETRS: order of
// "CcRr"), on host or device pointers alike, before a device is touched.  f: the factors; ins: every input pointer beside
// them (none; ipiv) is there.  *empty: n == 0 or k == 0, which is decided before the pointers are looked at.
static int bjacobi_apply_check_args(bool flags_ok, int p, int max_p, int64_t n, int k, const double *f, int ldf, int64_t stride,
                                    bool ins, const double *x, int64_t ldx, int fpe, bool *empty)
{
    *empty = false;
    if (!flags_ok) return (int)hipErrorInvalidValue;
    if (n < 0 || k < 0 || p < 0 || p > max_p || (p < 1 && n > 0) || fpe < 0 || ldx < k) return (int)hipErrorInvalidValue;
    if (ldf < (p > 1 ? p : 1)) return (int)hipErrorInvalidValue;
    if (p > 0 && n > p && stride < (int64_t)ldf * p) return (int)hipErrorInvalidValue;   // more than one block
    if (fpe >= 9) return EXBLAS_UNSUPPORTED;
    *empty = n == 0 || k == 0;
    if (!*empty && (!f || !ins || !x)) return (int)hipErrorInvalidValue;
    return 0;
}

static int potrs_batched_check_args(char uplo, char sweep, int p, int64_t n, int k, const double *r, int ldr, int64_t stride,
                                    const double *x, int64_t ldx, int fpe, bool *empty)
{
    return bjacobi_apply_check_args(one_of(uplo, "LlUu") && one_of(sweep, "12Bb"), p, EXBLAS_POTRF_BATCHED_MAX_P, n, k, r, ldr,
                                    stride, true, x, ldx, fpe, empty);
}

static int getrs_batched_check_args(char order, int p, int64_t n, int k, const double *lu, int ldlu, int64_t stride,
                                    const int *ipiv, const double *x, int64_t ldx, int fpe, bool *empty)
{
    return bjacobi_apply_check_args(one_of(order, "CcRr"), p, EXBLAS_GETRF_BATCHED_MAX_P, n, k, lu, ldlu, stride,
                                    ipiv != nullptr, x, ldx, fpe, empty);
}

static int expotrs_batched_on(Ctx &c, char uplo, char sweep, int p, int64_t n, int k, const double *d_r, int ldr,
                              int64_t stride, double *d_x, int64_t ldx, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // an empty call goes on: it counts as the device's last one, and the dispatch launches nothing
    if (int rc = potrs_batched_check_args(uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)expotrs_batched_dispatch(c, uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, early_exit, round_mode(),
                                         st);
}

static int exgetrf_batched_on(Ctx &c, char order, int p, int64_t batch, double *d_a, int lda, int64_t stride, int *d_ipiv,
                              int *d_info, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // an empty call goes on: it counts as the device's last one, and the dispatch launches nothing
    if (int rc = getrf_batched_check_args(order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exgetrf_batched_dispatch(c, order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, early_exit, round_mode(),
                                         st);
}

static int exgetrs_batched_on(Ctx &c, char order, int p, int64_t n, int k, const double *d_lu, int ldlu, int64_t stride,
                              const int *d_ipiv, double *d_x, int64_t ldx, int fpe, int early_exit, hipStream_t st)
{
    bool empty;   // an empty call goes on: it counts as the device's last one, and the dispatch launches nothing
    if (int rc = getrs_batched_check_args(order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, &empty)) return rc;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exgetrs_batched_dispatch(c, order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, early_exit,
                                         round_mode(), st);
}

static int exgemm_on(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *d_a, int lda,
                     const double *d_b, int ldb, double beta, double *d_c, int ldc, int fpe, int early_exit,
                     hipStream_t st, const GemmChunks *chunks = nullptr)
{
    if (fpe < 0) return (int)hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.layer < MAX_LAYERS) g_last_layer[c.device] = c.layer;
    return (int)exgemm_dispatch(c, transa, transb, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, fpe,
                                early_exit, round_mode(), st, chunks);
}

int exblas_exsum_segmented_dev(const double *d_values, const int64_t *d_offsets, int64_t nseg, int fpe, int early_exit,
                               void *stream, double *d_out)
{
    if (fpe < 0) return (int)hipErrorInvalidValue;
    ctx(-1);
    return (int)exsum_segmented_dispatch(d_values, (const long long *)d_offsets, nseg, fpe, early_exit, round_mode(),
                                         (hipStream_t)stream, d_out);
}

int exblas_finalize_dev(const int64_t *d_digit_sets, int nsets, uint32_t flags_or, void *stream, int64_t *d_out)
{
    ctx(-1);
    return (int)finalize_sets((const long long *)d_digit_sets, nsets, flags_or, (hipStream_t)stream,
                              (long long *)d_out);
}

int exblas_extrsv_last_slow_rows(void)
{
    Ctx &c = ctx(-1, g_last_layer[current_device()]);
    std::lock_guard<std::mutex> lk(c.mu);
    int v[4] = {0, 0, 0, 0};
    if (!c.ws || c.ws_bytes < sizeof(v)) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(v, c.ws, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v[2];
}

}  // extern "C"
int exb::exbdot_merged_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
                           double *d_c, int64_t ldc, int fpe, int early_exit, hipStream_t st, const BdotMerge *merge)
{
    bool empty;
    const int rc = bdot_check_args(mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, &empty);
    if (rc) return rc;
    if (fpe == 1) return (int)hipErrorInvalidValue;   // plain fp64 sums have no digit sets to merge
    if (empty || (early_exit && fpe > 8)) return 0;    // (the silent return of exblas_exbdot_dev)
    Ctx &c = ctx(-1);
    std::lock_guard<std::mutex> lk(c.mu);
    return exbdot_merge_dispatch(c, mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, early_exit, round_mode(), merge, st);
}
int exb::exgemm_chunked_dev(char transa, char transb, int m, int n, int k, double alpha, const double *d_a, int lda,
                            const double *d_b, int ldb, double beta, double *d_c, int ldc, int fpe, int early_exit,
                            hipStream_t st, const GemmChunks *chunks)
{
    return exgemm_on(ctx(-1), transa, transb, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, fpe, early_exit, st,
                     chunks);
}

// ---- context handles: independent accumulators, flags and workspace per caller-owned handle --------------------
struct exblas_ctx {
    exb::Ctx c;
};
// the calling thread must be on the handle's device (like any stream or buffer of that device)
static bool wrong_device(exblas_ctx *h) { return h && current_device() != h->c.device; }
// the handle's context; NULL: the device's default context, created if need be
static Ctx *handle_ctx(exblas_ctx *h)
{
    if (!h) return &ctx(-1);
    return wrong_device(h) ? nullptr : &h->c;
}
extern "C" {

int exblas_ctx_create(exblas_ctx_t **out)
{
    if (!out) return (int)hipErrorInvalidValue;
    ctx(-1);  // the device's default context first: a handle inherits the knobs set through the API
    exblas_ctx *h = new exblas_ctx;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        init_ctx(h->c, current_device(), MAX_LAYERS);  // layer >= 1: inherits; >= MAX_LAYERS: not one of the static ones
    }
    *out = h;
    return 0;
}

int exblas_ctx_destroy(exblas_ctx_t *h)
{
    if (!h) return 0;
    Ctx &c = h->c;
    int prev = 0;
    (void)hipGetDevice(&prev);
    hipError_t first = hipSetDevice(c.device);
    hipError_t e = hipDeviceSynchronize();  // work enqueued on the handle may still be running
    if (first == hipSuccess) first = e;
    auto rel = [&](void *p) {
        if (!p) return;
        hipError_t e2 = hipFree(p);
        if (first == hipSuccess) first = e2;
    };
    rel(c.gacc_all);
    rel(c.gflags_all);
    rel(c.d_record);
    for (void *p : c.stage) rel(p);
    for (void *p : c.retired) rel(p);
    rel(c.ws);
    if (c.h_record) (void)hipHostFree(c.h_record);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    (void)hipSetDevice(prev);
    delete h;
    return (int)first;
}

#define EXB_HANDLE(h)              \
    Ctx *cp = handle_ctx(h);       \
    if (!cp) return (int)hipErrorInvalidDevice

int exblas_exsum_accumulate_ctx(exblas_ctx_t *h, const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                                void *stream)
{
    EXB_HANDLE(h);
    return exsum_accumulate_on(*cp, d_a, n, inca, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exdot_accumulate_ctx(exblas_ctx_t *h, const double *d_a, int64_t inca, const double *d_b, int64_t incb,
                                int64_t n, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return exdot_accumulate_on(*cp, d_a, inca, d_b, incb, n, fpe, early_exit, (hipStream_t)stream);
}

int exblas_finish_ctx(exblas_ctx_t *h, void *stream, int64_t *d_out)
{
    EXB_HANDLE(h);
    return finish_on(*cp, (hipStream_t)stream, d_out);
}

int exblas_exsum_ctx(exblas_ctx_t *h, const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream,
                     int64_t *d_out)
{
    EXB_HANDLE(h);
    int rc = exsum_accumulate_on(*cp, d_a, n, inca, fpe, early_exit, (hipStream_t)stream);
    return rc ? rc : finish_on(*cp, (hipStream_t)stream, d_out);
}

int exblas_exdot_ctx(exblas_ctx_t *h, const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n, int fpe,
                     int early_exit, void *stream, int64_t *d_out)
{
    EXB_HANDLE(h);
    int rc = exdot_accumulate_on(*cp, d_a, inca, d_b, incb, n, fpe, early_exit, (hipStream_t)stream);
    return rc ? rc : finish_on(*cp, (hipStream_t)stream, d_out);
}

// (the refusals come first: a refused call must not create the default context)
int exblas_exsum_lp_accumulate_ctx(exblas_ctx_t *h, int dtype, const void *d_a, int64_t n, int64_t inca, int fpe,
                                   int early_exit, void *stream)
{
    if (int rc = lp_refused(dtype, d_a, inca, nullptr, 1, n, fpe)) return rc;
    EXB_HANDLE(h);
    return exsum_lp_accumulate_on(*cp, dtype, d_a, n, inca, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exdot_lp_accumulate_ctx(exblas_ctx_t *h, int dtype, const void *d_a, int64_t inca, const void *d_b,
                                   int64_t incb, int64_t n, int fpe, int early_exit, void *stream)
{
    if (int rc = lp_refused(dtype, d_a, inca, d_b, incb, n, fpe)) return rc;
    EXB_HANDLE(h);
    return exdot_lp_accumulate_on(*cp, dtype, d_a, inca, d_b, incb, n, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exsum_lp_ctx(exblas_ctx_t *h, int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                        void *stream, int64_t *d_out)
{
    int rc = exblas_exsum_lp_accumulate_ctx(h, dtype, d_a, n, inca, fpe, early_exit, stream);
    return rc ? rc : exblas_finish_ctx(h, stream, d_out);
}

int exblas_exdot_lp_ctx(exblas_ctx_t *h, int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb,
                        int64_t n, int fpe, int early_exit, void *stream, int64_t *d_out)
{
    int rc = exblas_exdot_lp_accumulate_ctx(h, dtype, d_a, inca, d_b, incb, n, fpe, early_exit, stream);
    return rc ? rc : exblas_finish_ctx(h, stream, d_out);
}

// (no state of the context is used: the handle only says which device the pointers belong to)
int exblas_round_records_ctx(exblas_ctx_t *h, const int64_t *d_records, int64_t count, int64_t stride_words, int dtype,
                             void *d_out, void *stream)
{
    if (int rc = round_records_refused(d_records, count, stride_words, dtype, d_out)) return rc;
    if (count == 0) return 0;
    EXB_HANDLE(h);
    return (int)round_records_dispatch((const long long *)d_records, count, stride_words, dtype, d_out, (hipStream_t)stream);
}

int exblas_round_digits_host(const int64_t *digits68, int dtype, uint64_t *bits)
{
    if (!digits68 || !bits || !dtype_known(dtype)) return (int)hipErrorInvalidValue;
    long long v[NL];
    for (int i = 0; i < NL; ++i) v[i] = digits68[i];
    *bits = round_digits_to(v, dtype);
    return 0;
}

int exblas_exgemv_ctx(exblas_ctx_t *h, char transa, int m, int n, double alpha, const double *d_a, int lda,
                      const double *d_x, int incx, double beta, double *d_y, int incy, int fpe, int early_exit,
                      void *stream)
{
    EXB_HANDLE(h);
    return exgemv_on(*cp, transa, m, n, alpha, d_a, lda, d_x, incx, beta, d_y, incy, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exspmv_csr_ctx(exblas_ctx_t *h, int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                          const double *d_val, double alpha, const double *d_x, double beta, double *d_y, int fpe,
                          int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return exspmv_on(*cp, m, n, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, beta, d_y, fpe, early_exit,
                     (hipStream_t)stream);
}

int exblas_exspmm_csr_ctx(exblas_ctx_t *h, int m, int n, int k, int index_bits, const void *d_row_ptr,
                          const void *d_col_idx, const double *d_val, double alpha, const double *d_x, int64_t ldx,
                          double beta, double *d_y, int64_t ldy, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return exspmm_on(*cp, m, n, k, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, ldx, beta, d_y, ldy, fpe,
                     early_exit, (hipStream_t)stream);
}

// The narrow CSR entries refuse bad arguments before they need a device (as the narrow reductions above)
int exblas_exspmv_csr_lp_ctx(exblas_ctx_t *h, int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                             int val_dtype, const void *d_val, double alpha, int vec_dtype, const void *d_x, double beta,
                             void *d_y, int fpe, int early_exit, void *stream)
{
    if (int rc = csr_lp_precheck(m, n, 1, index_bits, d_row_ptr, val_dtype, d_val, vec_dtype, d_x, 1, d_y, 1, fpe)) return rc;
    EXB_HANDLE(h);
    return exspmv_lp_on(*cp, m, n, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype, d_x, beta, d_y, fpe,
                        early_exit, (hipStream_t)stream);
}

int exblas_exspmm_csr_lp_ctx(exblas_ctx_t *h, int m, int n, int k, int index_bits, const void *d_row_ptr,
                             const void *d_col_idx, int val_dtype, const void *d_val, double alpha, int vec_dtype,
                             const void *d_x, int64_t ldx, double beta, void *d_y, int64_t ldy, int fpe, int early_exit,
                             void *stream)
{
    if (int rc = csr_lp_precheck(m, n, k, index_bits, d_row_ptr, val_dtype, d_val, vec_dtype, d_x, ldx, d_y, ldy, fpe))
        return rc;
    EXB_HANDLE(h);
    return exspmm_lp_on(*cp, m, n, k, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype, d_x, ldx, beta,
                        d_y, ldy, fpe, early_exit, (hipStream_t)stream);
}

// The accumulator rounding of the narrow sparse products on the CPU: the leading bit, the 64 bits from it down and "anything
// below" are taken from the digits one after the other (sp_pick_to, spmv_common.hip.h, takes them with the wave), then
// round_window_to rounds them -- so the CPU suite can hold that function to round_digits_to and the integer model.
int exblas_round_window_host(const int64_t *digits68, int dtype, uint64_t *bits)
{
    if (!digits68 || !bits || !dtype_known(dtype)) return (int)hipErrorInvalidValue;
    const bool neg = digits68[NL - 1] < 0;
    unsigned mag[NL];
    unsigned long long carry = 1;
    for (int i = 0; i < NL; ++i) {
        const unsigned d = (unsigned)digits68[i];
        if (!neg) {
            mag[i] = d;
        } else {
            const unsigned long long t = (unsigned long long)(~d) + carry;
            mag[i] = (unsigned)t;
            carry = t >> 32;
        }
    }
    int tp = NL - 1;
    while (tp >= 0 && mag[tp] == 0) --tp;
    *bits = 0;
    if (tp < 0) return 0;
    int z = 0;
    while (mag[z] == 0) ++z;
    const unsigned mt = mag[tp], ma = tp >= 1 ? mag[tp - 1] : 0u, mb = tp >= 2 ? mag[tp - 2] : 0u;
    const int lz = __builtin_clz(mt);
    unsigned long long w = ((unsigned long long)mt << 32) | ma;
    unsigned rest = mb;
    if (lz) {
        w = (w << lz) | (unsigned long long)(mb >> (32 - lz));
        rest = mb << lz;
    }
    *bits = round_window_to(neg, 32 * tp + 31 - lz, w, rest != 0 || z < tp - 2, dtype);
    return 0;
}

int exblas_round_interval_host(double res, double bound, int dtype, uint64_t *bits)
{
    if (!bits || !dtype_known(dtype)) return -(int)hipErrorInvalidValue;   // (1 and 0 are answers)
    unsigned long long b = 0;
    const int ok = round_interval_to(res, bound, dtype, &b);
    *bits = ok ? b : 0;
    return ok;
}

// The three ExBDOT entries refuse bad arguments, or return 0 for an empty problem, before they need a device: the check
// comes before the default context is created (a handle on the wrong device is still refused first).
int exblas_exbdot_ctx(exblas_ctx_t *h, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx,
                      const double *d_y, int64_t ldy, double *d_c, int64_t ldc, int fpe, int early_exit, void *stream)
{
    if (wrong_device(h)) return (int)hipErrorInvalidDevice;
    bool empty;
    const int rc = bdot_check_args(mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, &empty);
    if (rc || empty) return rc;
    return exbdot_on(h ? h->c : ctx(-1), mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exbdot_export_ctx(exblas_ctx_t *h, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx,
                             const double *d_y, int64_t ldy, int64_t *d_sets, int fpe, int early_exit, void *stream)
{
    if (wrong_device(h)) return (int)hipErrorInvalidDevice;
    bool empty;
    const int rc = bdot_export_check(mode, n, p, q, d_x, ldx, d_y, ldy, d_sets, fpe, early_exit, &empty);
    if (rc || empty) return rc;
    return exbdot_export_on(h ? h->c : ctx(-1), mode, n, p, q, d_x, ldx, d_y, ldy, d_sets, fpe, early_exit,
                            (hipStream_t)stream);
}

// (the round uses nothing of the context: the handle is checked, and the form is there for symmetry with the export;
// without a handle the default context is still created, so that a process without a device ends as everywhere else)
int exblas_exbdot_round_ctx(exblas_ctx_t *h, char mode, int p, int q, const int64_t *d_sets, int nsets, double *d_c,
                            int64_t ldc, void *stream)
{
    if (wrong_device(h)) return (int)hipErrorInvalidDevice;
    bool empty;
    const int rc = bdot_round_check(mode, p, q, d_sets, nsets, d_c, ldc, &empty);
    if (rc || empty) return rc;
    if (!h) ctx(-1);
    return (int)exbdot_round_dispatch(mode, p, q, (const long long *)d_sets, nsets, d_c, ldc, round_mode(),
                                      (hipStream_t)stream);
}

int exblas_exsptrsv_csr_ctx(exblas_ctx_t *h, char uplo, char diag, int m, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return exsptrsv_on(*cp, uplo, diag, m, index_bits, d_row_ptr, d_col_idx, d_val, d_x, fpe, early_exit,
                       (hipStream_t)stream);
}

int exblas_exspilu0_csr_ctx(exblas_ctx_t *h, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                            const double *d_val, double *d_lu, int64_t *d_info, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return exspilu0_on(*cp, m, index_bits, d_row_ptr, d_col_idx, d_val, d_lu, d_info, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exspic0_csr_ctx(exblas_ctx_t *h, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                           const double *d_val, double *d_ll, int64_t *d_info, int fpe, int early_exit, void *stream)
{
    if (spic0_args_bad(m, index_bits, d_row_ptr, d_info, fpe)) return (int)hipErrorInvalidValue;
    EXB_HANDLE(h);
    return exspic0_on(*cp, m, index_bits, d_row_ptr, d_col_idx, d_val, d_ll, d_info, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exsptrsm_csr_ctx(exblas_ctx_t *h, char uplo, char diag, int m, int k, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int64_t ldx, int fpe, int early_exit,
                            void *stream)
{
    EXB_HANDLE(h);
    return exsptrsm_on(*cp, uplo, diag, m, k, index_bits, d_row_ptr, d_col_idx, d_val, d_x, ldx, fpe, early_exit,
                       (hipStream_t)stream);
}

int exblas_extrsv_ctx(exblas_ctx_t *h, char uplo, char transa, char diag, int n, const double *d_a, int lda, double *d_x,
                      int incx, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return extrsv_on(*cp, uplo, transa, diag, n, d_a, lda, d_x, incx, fpe, early_exit, (hipStream_t)stream);
}

int exblas_extrsm_ctx(exblas_ctx_t *h, char uplo, char transa, char diag, int n, int k, const double *d_a, int lda,
                      double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    EXB_HANDLE(h);
    return extrsm_on(*cp, uplo, transa, diag, n, k, d_a, lda, d_x, ldx, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exbgemm_ctx(exblas_ctx_t *h, int64_t n, int p, int q, double alpha, const double *d_x, int64_t ldx,
                       const double *d_c, int64_t ldc, double beta, double *d_y, int64_t ldy, int fpe, int early_exit,
                       void *stream)
{
    EXB_HANDLE(h);
    return exbgemm_on(*cp, n, p, q, alpha, d_x, ldx, d_c, ldc, beta, d_y, ldy, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exbtrsm_ctx(exblas_ctx_t *h, char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *d_t,
                       int ldt, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = btrsm_check_args(uplo, transt, diag, n, p, d_t, ldt, d_x, ldx, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return exbtrsm_on(*cp, uplo, transt, diag, n, p, alpha, d_t, ldt, d_x, ldx, fpe, early_exit, (hipStream_t)stream);
}

int exblas_expotrf_ctx(exblas_ctx_t *h, char uplo, int p, double *d_g, int ldg, int *d_info, int fpe, int early_exit,
                       void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = potrf_check_args(uplo, p, d_g, ldg, d_info, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return expotrf_on(*cp, uplo, p, d_g, ldg, d_info, fpe, early_exit, (hipStream_t)stream);
}

int exblas_expotrf_batched_ctx(exblas_ctx_t *h, char uplo, int p, int64_t batch, double *d_g, int ldg, int64_t stride,
                               int *d_info, int fpe, int early_exit, void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = potrf_batched_check_args(uplo, p, batch, d_g, ldg, stride, d_info, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return expotrf_batched_on(*cp, uplo, p, batch, d_g, ldg, stride, d_info, fpe, early_exit, (hipStream_t)stream);
}

int exblas_expotrs_batched_ctx(exblas_ctx_t *h, char uplo, char sweep, int p, int64_t n, int k, const double *d_r, int ldr,
                               int64_t stride, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = potrs_batched_check_args(uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return expotrs_batched_on(*cp, uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exgetrf_batched_ctx(exblas_ctx_t *h, char order, int p, int64_t batch, double *d_a, int lda, int64_t stride,
                               int *d_ipiv, int *d_info, int fpe, int early_exit, void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = getrf_batched_check_args(order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return exgetrf_batched_on(*cp, order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, early_exit, (hipStream_t)stream);
}

int exblas_exgetrs_batched_ctx(exblas_ctx_t *h, char order, int p, int64_t n, int k, const double *d_lu, int ldlu,
                               int64_t stride, const int *d_ipiv, double *d_x, int64_t ldx, int fpe, int early_exit,
                               void *stream)
{
    bool empty;   // a bad argument is refused before the context, and with it the device, is looked up
    if (int rc = getrs_batched_check_args(order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, &empty)) return rc;
    EXB_HANDLE(h);
    return exgetrs_batched_on(*cp, order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, early_exit,
                              (hipStream_t)stream);
}

int exblas_exgemm_ctx(exblas_ctx_t *h, char transa, char transb, int m, int n, int k, double alpha, const double *d_a,
                      int lda, const double *d_b, int ldb, double beta, double *d_c, int ldc, int fpe, int early_exit,
                      void *stream)
{
    EXB_HANDLE(h);
    return exgemm_on(*cp, transa, transb, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, fpe, early_exit,
                     (hipStream_t)stream);
}

int exblas_reserve_workspace_ctx(exblas_ctx_t *h, size_t bytes)
{
    EXB_HANDLE(h);
    std::lock_guard<std::mutex> lk(cp->mu);
    hipError_t e = hipSuccess;
    workspace(*cp, bytes, nullptr, &e);
    return (int)e;
}

size_t exblas_workspace_bytes_ctx(exblas_ctx_t *h)
{
    Ctx *cp = handle_ctx(h);
    if (!cp) return 0;
    std::lock_guard<std::mutex> lk(cp->mu);
    return cp->ws_bytes;
}

int exblas_last_gemm_info_ctx(exblas_ctx_t *h, int *out8)
{
    EXB_HANDLE(h);
    return last_gemm_info_on(*cp, out8);
}
#undef EXB_HANDLE

// ---- the *_dev entries: the same call on the NULL handle, the device's default context -------------------------
int exblas_exsum_accumulate_dev(const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream)
{
    return exblas_exsum_accumulate_ctx(nullptr, d_a, n, inca, fpe, early_exit, stream);
}
int exblas_exdot_accumulate_dev(const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n, int fpe,
                                int early_exit, void *stream)
{
    return exblas_exdot_accumulate_ctx(nullptr, d_a, inca, d_b, incb, n, fpe, early_exit, stream);
}
int exblas_finish_dev(void *stream, int64_t *d_out) { return exblas_finish_ctx(nullptr, stream, d_out); }
int exblas_exsum_dev(const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream, int64_t *d_out)
{
    return exblas_exsum_ctx(nullptr, d_a, n, inca, fpe, early_exit, stream, d_out);
}
int exblas_exdot_dev(const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n, int fpe,
                     int early_exit, void *stream, int64_t *d_out)
{
    return exblas_exdot_ctx(nullptr, d_a, inca, d_b, incb, n, fpe, early_exit, stream, d_out);
}
int exblas_exsum_lp_accumulate_dev(int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream)
{
    return exblas_exsum_lp_accumulate_ctx(nullptr, dtype, d_a, n, inca, fpe, early_exit, stream);
}
int exblas_exdot_lp_accumulate_dev(int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb, int64_t n,
                                   int fpe, int early_exit, void *stream)
{
    return exblas_exdot_lp_accumulate_ctx(nullptr, dtype, d_a, inca, d_b, incb, n, fpe, early_exit, stream);
}
int exblas_exsum_lp_dev(int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream,
                        int64_t *d_out)
{
    return exblas_exsum_lp_ctx(nullptr, dtype, d_a, n, inca, fpe, early_exit, stream, d_out);
}
int exblas_exdot_lp_dev(int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb, int64_t n, int fpe,
                        int early_exit, void *stream, int64_t *d_out)
{
    return exblas_exdot_lp_ctx(nullptr, dtype, d_a, inca, d_b, incb, n, fpe, early_exit, stream, d_out);
}
int exblas_round_records_dev(const int64_t *d_records, int64_t count, int64_t stride_words, int dtype, void *d_out,
                             void *stream)
{
    return exblas_round_records_ctx(nullptr, d_records, count, stride_words, dtype, d_out, stream);
}
int exblas_exgemv_dev(char transa, int m, int n, double alpha, const double *d_a, int lda, const double *d_x,
                      int incx, double beta, double *d_y, int incy, int fpe, int early_exit, void *stream)
{
    return exblas_exgemv_ctx(nullptr, transa, m, n, alpha, d_a, lda, d_x, incx, beta, d_y, incy, fpe, early_exit, stream);
}
int exblas_extrsv_dev(char uplo, char transa, char diag, int n, const double *d_a, int lda, double *d_x, int incx,
                      int fpe, int early_exit, void *stream)
{
    return exblas_extrsv_ctx(nullptr, uplo, transa, diag, n, d_a, lda, d_x, incx, fpe, early_exit, stream);
}
int exblas_extrsm_dev(char uplo, char transa, char diag, int n, int k, const double *d_a, int lda, double *d_x,
                      int64_t ldx, int fpe, int early_exit, void *stream)
{
    return exblas_extrsm_ctx(nullptr, uplo, transa, diag, n, k, d_a, lda, d_x, ldx, fpe, early_exit, stream);
}
int exblas_exbtrsm_dev(char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *d_t, int ldt,
                       double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    return exblas_exbtrsm_ctx(nullptr, uplo, transt, diag, n, p, alpha, d_t, ldt, d_x, ldx, fpe, early_exit, stream);
}

int exblas_expotrf_dev(char uplo, int p, double *d_g, int ldg, int *d_info, int fpe, int early_exit, void *stream)
{
    return exblas_expotrf_ctx(nullptr, uplo, p, d_g, ldg, d_info, fpe, early_exit, stream);
}

int exblas_expotrf_batched_dev(char uplo, int p, int64_t batch, double *d_g, int ldg, int64_t stride, int *d_info, int fpe,
                               int early_exit, void *stream)
{
    return exblas_expotrf_batched_ctx(nullptr, uplo, p, batch, d_g, ldg, stride, d_info, fpe, early_exit, stream);
}

int exblas_expotrs_batched_dev(char uplo, char sweep, int p, int64_t n, int k, const double *d_r, int ldr, int64_t stride,
                               double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    return exblas_expotrs_batched_ctx(nullptr, uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, early_exit, stream);
}

int exblas_exgetrf_batched_dev(char order, int p, int64_t batch, double *d_a, int lda, int64_t stride, int *d_ipiv, int *d_info,
                               int fpe, int early_exit, void *stream)
{
    return exblas_exgetrf_batched_ctx(nullptr, order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, early_exit, stream);
}

int exblas_exgetrs_batched_dev(char order, int p, int64_t n, int k, const double *d_lu, int ldlu, int64_t stride,
                               const int *d_ipiv, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream)
{
    return exblas_exgetrs_batched_ctx(nullptr, order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, early_exit, stream);
}

int exblas_exbgemm_dev(int64_t n, int p, int q, double alpha, const double *d_x, int64_t ldx, const double *d_c,
                       int64_t ldc, double beta, double *d_y, int64_t ldy, int fpe, int early_exit, void *stream)
{
    return exblas_exbgemm_ctx(nullptr, n, p, q, alpha, d_x, ldx, d_c, ldc, beta, d_y, ldy, fpe, early_exit, stream);
}
int exblas_exgemm_dev(char transa, char transb, int m, int n, int k, double alpha, const double *d_a, int lda,
                      const double *d_b, int ldb, double beta, double *d_c, int ldc, int fpe, int early_exit,
                      void *stream)
{
    return exblas_exgemm_ctx(nullptr, transa, transb, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, fpe, early_exit,
                             stream);
}
int exblas_exspmv_csr_dev(int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                          const double *d_val, double alpha, const double *d_x, double beta, double *d_y, int fpe,
                          int early_exit, void *stream)
{
    return exblas_exspmv_csr_ctx(nullptr, m, n, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, beta, d_y, fpe,
                                 early_exit, stream);
}
int exblas_exspmv_csr_lp_dev(int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx, int val_dtype,
                             const void *d_val, double alpha, int vec_dtype, const void *d_x, double beta, void *d_y, int fpe,
                             int early_exit, void *stream)
{
    return exblas_exspmv_csr_lp_ctx(nullptr, m, n, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype, d_x,
                                    beta, d_y, fpe, early_exit, stream);
}
int exblas_exspmm_csr_lp_dev(int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                             int val_dtype, const void *d_val, double alpha, int vec_dtype, const void *d_x, int64_t ldx,
                             double beta, void *d_y, int64_t ldy, int fpe, int early_exit, void *stream)
{
    return exblas_exspmm_csr_lp_ctx(nullptr, m, n, k, index_bits, d_row_ptr, d_col_idx, val_dtype, d_val, alpha, vec_dtype,
                                    d_x, ldx, beta, d_y, ldy, fpe, early_exit, stream);
}
int exblas_exspmm_csr_dev(int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                          const double *d_val, double alpha, const double *d_x, int64_t ldx, double beta, double *d_y,
                          int64_t ldy, int fpe, int early_exit, void *stream)
{
    return exblas_exspmm_csr_ctx(nullptr, m, n, k, index_bits, d_row_ptr, d_col_idx, d_val, alpha, d_x, ldx, beta, d_y, ldy,
                                 fpe, early_exit, stream);
}
int exblas_exspilu0_csr_dev(int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                            double *d_lu, int64_t *d_info, int fpe, int early_exit, void *stream)
{
    return exblas_exspilu0_csr_ctx(nullptr, m, index_bits, d_row_ptr, d_col_idx, d_val, d_lu, d_info, fpe, early_exit, stream);
}
int exblas_exspic0_csr_dev(int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                           double *d_ll, int64_t *d_info, int fpe, int early_exit, void *stream)
{
    return exblas_exspic0_csr_ctx(nullptr, m, index_bits, d_row_ptr, d_col_idx, d_val, d_ll, d_info, fpe, early_exit, stream);
}

int exblas_exsptrsv_csr_dev(char uplo, char diag, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                            const double *d_val, double *d_x, int fpe, int early_exit, void *stream)
{
    return exblas_exsptrsv_csr_ctx(nullptr, uplo, diag, m, index_bits, d_row_ptr, d_col_idx, d_val, d_x, fpe, early_exit,
                                   stream);
}
int exblas_exsptrsm_csr_dev(char uplo, char diag, int m, int k, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int64_t ldx, int fpe, int early_exit,
                            void *stream)
{
    return exblas_exsptrsm_csr_ctx(nullptr, uplo, diag, m, k, index_bits, d_row_ptr, d_col_idx, d_val, d_x, ldx, fpe,
                                   early_exit, stream);
}
int exblas_exbdot_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
                      double *d_c, int64_t ldc, int fpe, int early_exit, void *stream)
{
    return exblas_exbdot_ctx(nullptr, mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, early_exit, stream);
}
int exblas_exbdot_export_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y,
                             int64_t ldy, int64_t *d_sets, int fpe, int early_exit, void *stream)
{
    return exblas_exbdot_export_ctx(nullptr, mode, n, p, q, d_x, ldx, d_y, ldy, d_sets, fpe, early_exit, stream);
}
int exblas_exbdot_round_dev(char mode, int p, int q, const int64_t *d_sets, int nsets, double *d_c, int64_t ldc,
                            void *stream)
{
    return exblas_exbdot_round_ctx(nullptr, mode, p, q, d_sets, nsets, d_c, ldc, stream);
}
int exblas_reserve_workspace(size_t bytes) { return exblas_reserve_workspace_ctx(nullptr, bytes); }
size_t exblas_workspace_bytes(void) { return exblas_workspace_bytes_ctx(nullptr); }

// frees the parked blocks of a context whose lock is held; *first keeps the first failure
static void free_retired(Ctx &c, hipError_t *first)
{
    for (void *p : c.retired) {
        hipError_t e = hipFree(p);
        if (*first == hipSuccess) *first = e;
    }
    c.retired.clear();
}

int exblas_release_retired_workspaces(void)
{
    ctx(-1);
    hipError_t first = hipDeviceSynchronize();
    for_each_layer([&](Ctx &c) { free_retired(c, &first); });
    return (int)first;
}

int exblas_release_workspace(void)
{
    ctx(-1);
    hipError_t first = hipDeviceSynchronize();
    for_each_layer([&](Ctx &c) {
        free_retired(c, &first);
        if (c.ws) {
            hipError_t e = hipFree(c.ws);
            if (first == hipSuccess) first = e;
        }
        c.ws = nullptr;
        c.ws_bytes = 0;
        static_cast<CtxWsPtrs &>(c) = CtxWsPtrs();  // they pointed into the workspace
    });
    return (int)first;
}

// ---- host-pointer layer ---------------------------------------------------------------------

static size_t align_up(size_t b) { return (b + 255) & ~(size_t)255; }

static void check_fpe(int fpe)
{
    if (fpe < 0) {
        // cpu:ExSUM.cpp:25-28
        fprintf(stderr, "Size of floating-point expansion should be a positive number. Preferably, it should be "
                        "in the interval [2, 8]\n");
        exit(1);
    }
}

// ---- ExSUM / ExDOT of host vectors ---------------------------------------------------------------------------
// The reference's GPU backend copies the whole vector to ONE device per call (gpu:ExSUM.cpp:126), its CPU backend
// scatters slices from rank 0 to the other ranks (cpu:ExSUM.cpp:33-63).  Here one call spreads the vector over the
// GPUs of the node: every "virtual device" (a GPU, with a private host-layer context) gets a contiguous part, streams
// it through its own PCIe link in 64 MiB chunks (copy, accumulate kernel, copy, ...: bounded staging memory, the
// kernels hide behind the copies) and normalises its sum; the parts' 576-byte digit sets are then added and rounded
// once on the first device -- so the bits do not depend on how many GPUs took part.
static std::mutex g_host_mu;           // host-pointer calls are serialised process-wide (the reference's are not re-entrant at all)
static std::vector<int> g_host_devs;   // set by exblas_set_host_devices / EXBLAS_HOST_DEVICES; empty = default policy
static bool g_host_devs_env_read = false;
constexpr long long HOST_CHUNK_ELEMS = 8ll << 20;          // 64 MiB of doubles per copy
constexpr long long HOST_SPLIT_MIN_BYTES = 256ll << 20;    // smaller inputs stay on the current device

static std::vector<int> host_devices(long long bytes)
{
    if (!g_host_devs_env_read) {
        g_host_devs_env_read = true;
        const char *e = getenv("EXBLAS_HOST_DEVICES");  // "all", "current", or a list such as "0,1,2" / "0,0"
        if (e && *e && g_host_devs.empty()) {
            int ndev = exblas_hip_device_count();
            if (!strcmp(e, "all")) {
                for (int d = 0; d < ndev && d < MAX_LAYERS - 1; ++d) g_host_devs.push_back(d);
            } else if (strcmp(e, "current")) {
                for (const char *q = e; *q;) {
                    char *end;
                    long d = strtol(q, &end, 10);
                    if (end == q) break;
                    if (d >= 0 && d < ndev && (int)g_host_devs.size() < MAX_LAYERS - 1) g_host_devs.push_back((int)d);
                    q = *end ? end + 1 : end;
                }
            } else {
                g_host_devs.push_back(-1);  // current device only
            }
        }
    }
    std::vector<int> devs = g_host_devs;
    if (devs.empty()) {
        // default: one big call uses every GPU this process can see (8 PCIe links instead of 1); small ones do not
        // pay for waking the other devices.  NOT in a one-process-per-GPU job (a launcher's rank variables in the
        // environment, or a communicator created through exblas_comm_*): every rank sees all devices there, and a rank
        // that spread its host calls would create contexts and push PCIe traffic on its peers' GPUs -- the reference's
        // GPU backend uses exactly one device per call (gpu:ExSUM.cpp:86-126).
        static const bool rank_env = [] {
            for (const char *v : {"WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", "PMI_SIZE", "SLURM_NTASKS"}) {
                const char *e = getenv(v);
                if (e && atoi(e) > 1) return true;
            }
            return false;
        }();
        const int ndev = exblas_hip_device_count();
        if (bytes >= HOST_SPLIT_MIN_BYTES && ndev > 1 && !rank_env && !exb::g_comm_created.load())
            for (int d = 0; d < ndev && d < MAX_LAYERS - 1; ++d) devs.push_back(d);
        else
            devs.push_back(-1);
    }
    const int cur = current_device();
    for (int &d : devs)
        if (d < 0) d = cur;
    return devs;
}

struct HostPart {
    int dev = 0, layer = 1;
    long long i0 = 0, i1 = 0;
    int rc = 0;
    const char *what = "";
    bool want_ext = false;          // exdot over several parts: export the low / high digit sets instead of folding them
    std::vector<long long> ext;     // ... and bring them to the host (EXT_WORDS)
};

// one part of the vector(s) on one virtual device; leaves the part's record in the context's pinned h_record
static void host_reduce_part(HostPart &p, const double *a, long long inca, const double *b, long long incb, int fpe,
                             int early_exit)
{
    hipError_t e = hipSetDevice(p.dev);
    if (e != hipSuccess) { p.rc = (int)e; p.what = "hipSetDevice"; return; }
    Ctx &c = ctx(p.dev, p.layer);
    for (long long i = p.i0; i < p.i1 && !p.rc; i += HOST_CHUNK_ELEMS) {
        const long long cnt = std::min(HOST_CHUNK_ELEMS, p.i1 - i);
        const size_t spa = ((size_t)(cnt - 1) * (size_t)inca + 1) * sizeof(double);
        double *da, *db = nullptr;
        {
            std::lock_guard<std::mutex> lk(c.mu);
            da = (double *)stage_buf(c, 0, spa);
            if (b) db = (double *)stage_buf(c, 1, ((size_t)(cnt - 1) * (size_t)incb + 1) * sizeof(double));
        }
        // element count semantics of the GPU backend: a[offset + i*inca] (ExSUM.Superacc.cl:249-250); the touched
        // span of the chunk is copied like gpu:ExSUM.cpp:126 copies the whole vector
        e = hipMemcpyAsync(da, a + i * inca, spa, hipMemcpyHostToDevice, c.stream);
        if (e == hipSuccess && b)
            e = hipMemcpyAsync(db, b + i * incb, ((size_t)(cnt - 1) * (size_t)incb + 1) * sizeof(double),
                               hipMemcpyHostToDevice, c.stream);
        if (e != hipSuccess) { p.rc = (int)e; p.what = "hipMemcpyAsync"; return; }
        p.rc = b ? exdot_accumulate_on(c, da, inca, db, incb, cnt, fpe, early_exit, c.stream)
                 : exsum_accumulate_on(c, da, cnt, inca, fpe, early_exit, c.stream);
        p.what = "accumulate";
    }
    if (p.rc) return;
    long long *d_ext = nullptr;
    if (p.want_ext) {
        std::lock_guard<std::mutex> lk(c.mu);
        d_ext = (long long *)stage_buf(c, 2, sizeof(long long) * EXT_WORDS);
        p.rc = (int)finalize_groups(c, c.stream, c.d_record, d_ext);
    } else {
        p.rc = finish_on(c, c.stream, (int64_t *)c.d_record);
    }
    p.what = "finish";
    if (p.rc) return;
    e = hipMemcpyAsync(c.h_record, c.d_record, sizeof(long long) * OUT_WORDS, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess && d_ext) {
        p.ext.resize(EXT_WORDS);
        e = hipMemcpyAsync(p.ext.data(), d_ext, sizeof(long long) * EXT_WORDS, hipMemcpyDeviceToHost, c.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { p.rc = (int)e; p.what = "record copy"; }
}

static int host_reduce(long long n, const double *a, long long inca, const double *b, long long incb, int fpe,
                       int early_exit, int64_t *out_words)
{
    std::lock_guard<std::mutex> host_lock(g_host_mu);
    const int home = current_device();
    if (n < 0) n = 0;
    std::vector<int> devs = host_devices(n * (long long)sizeof(double) * (b ? 2 : 1));
    const int nv = (int)std::min<long long>((long long)devs.size(), std::max<long long>(1, n / 2));
    std::vector<HostPart> parts(nv);
    for (int v = 0; v < nv; ++v) {
        parts[v].dev = devs[v];
        parts[v].layer = 1 + v;
        parts[v].i0 = (n * v) / nv;
        parts[v].i1 = (n * (v + 1)) / nv;
        parts[v].want_ext = nv > 1 && b != nullptr;
    }
    if (nv == 1) {
        host_reduce_part(parts[0], a, inca, b, incb, fpe, early_exit);
    } else {
        std::vector<std::thread> th;
        for (int v = 0; v < nv; ++v)
            th.emplace_back([&, v] { host_reduce_part(parts[v], a, inca, b, incb, fpe, early_exit); });
        for (auto &t : th) t.join();
    }
    EXB_CHECK(hipSetDevice(home));
    for (auto &p : parts)
        if (p.rc) die(p.what, (hipError_t)p.rc, __FILE__, __LINE__);
    Ctx &c0 = ctx(parts[0].dev, parts[0].layer);
    if (nv > 1) {
        // add the parts' digit sets and round once, on the first device (exblas_finalize_dev's job in the *_dev layer)
        EXB_CHECK(hipSetDevice(c0.device));
        long long *d_sets;
        {
            std::lock_guard<std::mutex> lk(c0.mu);
            d_sets = (long long *)stage_buf(c0, 2, sizeof(long long) * (SET_WORDS * nv + EXT_WORDS));
        }
        for (int v = 0; v < nv; ++v) {
            Ctx &cv = ctx(parts[v].dev, parts[v].layer);
            EXB_CHECK(hipMemcpyAsync(d_sets + (size_t)v * SET_WORDS, cv.h_record + OUT_DIGITS,
                                     sizeof(long long) * SET_WORDS, hipMemcpyHostToDevice, c0.stream));
        }
        // exdot: the parts exported their low / high digit sets (products outside the double range, superacc.hip.h)
        // instead of folding them; their sums are folded once, like the multi-rank path does after its all-reduce
        long long *d_ext = nullptr;
        std::vector<long long> ext_sum;
        if (parts[0].want_ext) {
            ext_sum.assign(EXT_WORDS, 0);
            for (auto &p : parts)
                for (int i = 0; i < EXT_WORDS; ++i) ext_sum[i] += p.ext[i];
            d_ext = d_sets + (size_t)SET_WORDS * nv;
            EXB_CHECK(hipMemcpyAsync(d_ext, ext_sum.data(), sizeof(long long) * EXT_WORDS, hipMemcpyHostToDevice, c0.stream));
        }
        EXB_CHECK(finalize_sets(d_sets, nv, 0u, c0.stream, c0.d_record, d_ext));
        EXB_CHECK(hipMemcpyAsync(c0.h_record, c0.d_record, sizeof(long long) * OUT_WORDS, hipMemcpyDeviceToHost,
                                 c0.stream));
        EXB_CHECK(hipStreamSynchronize(c0.stream));
        EXB_CHECK(hipSetDevice(home));
    }
    memcpy(out_words, c0.h_record, sizeof(long long) * OUT_WORDS);
    return nv;
}

}  // extern "C"

// One call of the host-pointer layer below (everything but ExSUM / ExDOT): the layer-1 context of the current device,
// the process-wide lock of the layer, and the traffic around the one *_on call, which runs on the context's stream.
struct HostCall {
    Ctx &c = ctx(-1, 1);
    std::lock_guard<std::mutex> api_lock{g_host_mu};
    const char *who;
    explicit HostCall(const char *name) : who(name) {}
    void h2d(void *d, const void *h, size_t bytes)
    {
        if (bytes > 0) EXB_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c.stream));
    }
    // staging slot `slot` with room for `bytes`, the first `copy` bytes of `h` on their way into it
    double *in(int slot, size_t bytes, const void *h, size_t copy)
    {
        std::lock_guard<std::mutex> lk(c.mu);
        void *d = stage_buf(c, slot, bytes);
        h2d(d, h, copy);
        return (double *)d;
    }
    // the end of the call: dies when the routine returned rc != 0, else brings `bytes` at d back to h and waits for them
    int out(int rc, void *h, const void *d, size_t bytes)
    {
        if (rc) die(who, (hipError_t)rc, __FILE__, __LINE__);
        EXB_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c.stream));
        EXB_CHECK(hipStreamSynchronize(c.stream));
        return 0;
    }
};

extern "C" {

int exblas_set_host_devices(int count, const int *devices)
{
    std::lock_guard<std::mutex> host_lock(g_host_mu);
    const int ndev = exblas_hip_device_count();
    if (count < 0 || count > MAX_LAYERS - 1) return (int)hipErrorInvalidValue;
    for (int i = 0; i < count; ++i)
        if (devices[i] < 0 || devices[i] >= ndev) return (int)hipErrorInvalidDevice;
    g_host_devs.assign(devices, devices + count);  // count == 0: back to the default policy
    g_host_devs_env_read = true;
    return 0;
}

int exblas_exsum_record(int Ng, const double *ag, int inca, int offset, int fpe, int early_exit,
                        int64_t *out_words)
{
    check_fpe(fpe);
    host_reduce(Ng > 0 ? Ng : 0, ag + offset, inca > 0 ? inca : 1, nullptr, 1, fpe, early_exit, out_words);
    return 0;
}

int exblas_exdot_record(int Ng, const double *ag, int inca, int offseta, const double *bg, int incb, int offsetb,
                        int fpe, int early_exit, int64_t *out_words)
{
    check_fpe(fpe);
    host_reduce(Ng > 0 ? Ng : 0, ag + offseta, inca > 0 ? inca : 1, bg + offsetb, incb > 0 ? incb : 1, fpe, early_exit,
                out_words);
    return 0;
}

// Narrow ExSUM / ExDOT on host arrays: staged to the current device, the same *_on body, one device (b == nullptr: ExSUM)
static int host_lp(const char *who, int dtype, const void *a, int64_t inca, const void *b, int64_t incb, int64_t n, int fpe,
                   int early_exit, int64_t *out_words)
{
    if (int rc = lp_refused(dtype, a, inca, b, incb, n, fpe)) return rc;
    if (!out_words) return (int)hipErrorInvalidValue;
    HostCall hc(who);
    Ctx &c = hc.c;
    const size_t es = (size_t)dtype_bytes(dtype);
    const size_t abytes = n > 0 ? ((size_t)(n - 1) * (size_t)inca + 1) * es : 0;
    const size_t bbytes = (b && n > 0) ? ((size_t)(n - 1) * (size_t)incb + 1) * es : 0;
    const void *da = hc.in(0, abytes, a, abytes), *db = b ? hc.in(1, bbytes, b, bbytes) : nullptr;
    int rc = b ? exdot_lp_accumulate_on(c, dtype, da, inca, db, incb, n, fpe, early_exit, c.stream)
               : exsum_lp_accumulate_on(c, dtype, da, n, inca, fpe, early_exit, c.stream);
    if (!rc) rc = finish_on(c, c.stream, (int64_t *)c.d_record);
    return hc.out(rc, out_words, c.d_record, sizeof(long long) * OUT_WORDS);
}

int exblas_exsum_lp(int dtype, const void *a, int64_t n, int64_t inca, int fpe, int early_exit, int64_t *out_words)
{
    return host_lp("exblas_exsum_lp", dtype, a, inca, nullptr, 1, n, fpe, early_exit, out_words);
}

int exblas_exdot_lp(int dtype, const void *a, int64_t inca, const void *b, int64_t incb, int64_t n, int fpe, int early_exit,
                    int64_t *out_words)
{
    if (!b) return (int)hipErrorInvalidValue;
    return host_lp("exblas_exdot_lp", dtype, a, inca, b, incb, n, fpe, early_exit, out_words);
}

static double record_value(const int64_t *rec)
{
    double d;
    memcpy(&d, &rec[round_mode() ? EXBLAS_OUT_REFMODE : EXBLAS_OUT_EXACT], sizeof(d));
    return d;
}

double exblas_exsum(int Ng, const double *ag, int inca, int offset, int fpe, int early_exit)
{
    int64_t rec[EXBLAS_OUT_WORDS];
    exblas_exsum_record(Ng, ag, inca, offset, fpe, early_exit, rec);
    return record_value(rec);
}

double exblas_exdot(int Ng, const double *ag, int inca, int offseta, const double *bg, int incb, int offsetb,
                    int fpe, int early_exit)
{
    if (Ng <= 0) return 0.0;  // ExDOT.cpp:70-71
    int64_t rec[EXBLAS_OUT_WORDS];
    exblas_exdot_record(Ng, ag, inca, offseta, bg, incb, offsetb, fpe, early_exit, rec);
    return record_value(rec);
}

int exblas_exgemv(char transa, int m, int n, double alpha, const double *a, int lda, int offseta, const double *x,
                  int incx, int offsetx, double beta, double *y, int incy, int offsety, int fpe, int early_exit)
{
    check_fpe(fpe);
    if (m <= 0 || n <= 0) return 0;
    HostCall hc("exblas_exgemv");
    const bool trans = (transa == 'T' || transa == 't');
    const int rows = trans ? n : m, inner = trans ? m : n;
    const size_t abytes = (size_t)lda * (size_t)n * sizeof(double);  // column-major: n columns of lda
    const size_t xbytes = ((size_t)(inner - 1) * (size_t)incx + 1) * sizeof(double),
                 ybytes = ((size_t)(rows - 1) * (size_t)incy + 1) * sizeof(double);
    double *d_a = hc.in(0, abytes, a + offseta, abytes - (size_t)(lda - m) * sizeof(double));
    double *d_x = hc.in(1, xbytes, x + offsetx, xbytes);
    double *d_y = hc.in(2, ybytes, y + offsety, ybytes);
    return hc.out(exgemv_on(hc.c, transa, m, n, alpha, d_a, lda, d_x, incx, beta, d_y, incy, fpe, early_exit, hc.c.stream),
                  y + offsety, d_y, ybytes);
}

int exblas_extrsv(char uplo, char transa, char diag, int n, const double *a, int lda, int offseta, double *x,
                  int incx, int offsetx, int fpe, int early_exit)
{
    check_fpe(fpe);
    if (fpe >= 9) {
        fprintf(stderr, "exblas(hip): extrsv fpe = %d selects an iterative-refinement kernel the reference does not "
                        "ship (ExTRSV.cpp:91-120); nothing done\n", fpe);
        return -1;
    }
    if (n <= 0) return 0;
    HostCall hc("exblas_extrsv");
    const size_t abytes = ((size_t)lda * (size_t)(n - 1) + (size_t)n) * sizeof(double);  // n columns of lda
    const size_t xbytes = ((size_t)(n - 1) * (size_t)incx + 1) * sizeof(double);
    double *d_a = hc.in(0, abytes, a + offseta, abytes);
    double *d_x = hc.in(1, xbytes, x + offsetx, xbytes);
    return hc.out(extrsv_on(hc.c, uplo, transa, diag, n, d_a, lda, d_x, incx, fpe, early_exit, hc.c.stream), x + offsetx,
                  d_x, xbytes);
}

}  // extern "C"

// The host-pointer CSR call: Y (m x k, row stride ldy) from X (n x k, row stride ldx); ExSpMV is k = 1, ldx = ldy = 1.
// One staging block [row_ptr | col_idx | val | X | Y] goes to the device, launch(c, d_row_ptr, d_col_idx, d_val, d_x, d_y)
// runs the routine on the context's stream, and Y comes back.  ywords != 0: Y is that many words, not an m x k block.
// vsz, xsz: bytes of an element of val, and of X and Y (the narrow entries; launch still sees them as double pointers).
template <class Launch>
static int csr_host_call(const char *who, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                         const void *val, const void *x, int64_t ldx, void *y, int64_t ldy, int fpe,
                         Launch &&launch, size_t ywords = 0, size_t vsz = 8, size_t xsz = 8)
{
    bool empty;
    const int bad = csr_check_args(m, n, k, index_bits, row_ptr, (const double *)x, ldx, (const double *)y, ldy, fpe, &empty);
    if (bad || empty) return bad;
    // the entries the call reads: [0, max row_ptr); a negative row_ptr entry is refused
    const size_t isz = index_bits / 8;
    long long nnz = 0;
    for (int i = 0; i <= m; ++i) {
        const long long v = index_bits == 32 ? (long long)((const int32_t *)row_ptr)[i] : ((const int64_t *)row_ptr)[i];
        if (v < 0) return (int)hipErrorInvalidValue;
        if (v > nnz) nnz = v;
    }
    if (nnz > 0 && (!col_idx || !val)) return (int)hipErrorInvalidValue;
    HostCall hc(who);
    // whole rows of X and Y travel, padding included (the last row only up to its k-th entry)
    const size_t xspan = n > 0 ? (size_t)(n - 1) * (size_t)ldx + (size_t)k : 0;
    const size_t yspan = ywords ? ywords : (size_t)(m - 1) * (size_t)ldy + (size_t)k;
    const size_t b_rp = align_up((size_t)(m + 1) * isz), b_ci = align_up((size_t)nnz * isz),
                 b_val = align_up((size_t)nnz * vsz), b_x = align_up(xspan * xsz), b_y = align_up(yspan * xsz);
    char *d = (char *)hc.in(0, b_rp + b_ci + b_val + b_x + b_y, row_ptr, (size_t)(m + 1) * isz);
    char *d_val = d + b_rp + b_ci, *d_x = d_val + b_val, *d_y = d_x + b_x;
    hc.h2d(d + b_rp, col_idx, (size_t)nnz * isz);
    hc.h2d(d_val, val, (size_t)nnz * vsz);
    hc.h2d(d_x, x, xspan * xsz);
    hc.h2d(d_y, y, yspan * xsz);
    // the padding of Y comes back as it went
    return hc.out(launch(hc.c, (const void *)d, (const void *)(d + b_rp), (const double *)d_val, (const double *)d_x,
                         (double *)d_y),
                  y, d_y, yspan * xsz);
}

// what a host solve returns after its csr_host_call: the status of the layer-1 context's last solve
static int host_solve_status(const long long *CtxWsPtrs::*info_dev)
{
    Ctx &c = ctx(-1, 1);
    std::lock_guard<std::mutex> lk(c.mu);
    long long h[8];
    return solve_status(c.*info_dev, h);
}

// the shared CSR host path with Y = [factor | info]: nnz values (they travel both ways, so that a refused structure leaves
// the factor as it was) and the two info words behind them; `on` is exspilu0_on or exspic0_on
template <class On>
static int csr_factor_host(const char *who, const long long *CtxWsPtrs::*info_dev, int m, int index_bits, const void *row_ptr,
                           const void *col_idx, const double *val, double *out, int64_t *info, int fpe, On &&on)
{
    if (m < 0 || !info || (index_bits != 32 && index_bits != 64)) return (int)hipErrorInvalidValue;
    info[0] = info[1] = 0;
    if (m == 0) return fpe < 0 ? (int)hipErrorInvalidValue : 0;
    if (!row_ptr) return (int)hipErrorInvalidValue;
    long long nnz = 0;   // as csr_host_call counts them (it refuses a negative entry)
    for (int i = 0; i <= m; ++i)
        nnz = std::max(nnz, index_bits == 32 ? (long long)((const int32_t *)row_ptr)[i] : (long long)((const int64_t *)row_ptr)[i]);
    if (nnz > 0 && !out) return (int)hipErrorInvalidValue;
    std::vector<double> y((size_t)nnz + 2, 0.0);
    if (nnz > 0) memcpy(y.data(), out, (size_t)nnz * sizeof(double));
    const int rc = csr_host_call(
        who, m, 0, 1, index_bits, row_ptr, col_idx, val, nullptr, 1, y.data(), 1, fpe,
        [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *, double *d_y) {
            return on(c, m, index_bits, d_rp, d_ci, d_val, d_y, (int64_t *)(d_y + nnz), c.stream);
        },
        (size_t)nnz + 2);
    if (rc) return rc;
    if (nnz > 0) memcpy(out, y.data(), (size_t)nnz * sizeof(double));
    memcpy(info, y.data() + nnz, 2 * sizeof(int64_t));
    return host_solve_status(info_dev);
}

extern "C" {

int exblas_exspmv_csr(int m, int n, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                      double alpha, const double *x, double beta, double *y, int fpe, int early_exit)
{
    return csr_host_call("exblas_exspmv_csr", m, n, 1, index_bits, row_ptr, col_idx, val, x, 1, y, 1, fpe,
                         [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *d_x, double *d_y) {
                             return exspmv_on(c, m, n, index_bits, d_rp, d_ci, d_val, alpha, d_x, beta, d_y, fpe, early_exit,
                                              c.stream);
                         });
}

int exblas_exspmm_csr(int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                      double alpha, const double *x, int64_t ldx, double beta, double *y, int64_t ldy, int fpe,
                      int early_exit)
{
    return csr_host_call("exblas_exspmm_csr", m, n, k, index_bits, row_ptr, col_idx, val, x, ldx, y, ldy, fpe,
                         [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *d_x, double *d_y) {
                             return exspmm_on(c, m, n, k, index_bits, d_rp, d_ci, d_val, alpha, d_x, ldx, beta, d_y, ldy, fpe,
                                              early_exit, c.stream);
                         });
}

// the narrow products on host arrays stage through the current device as the fp64 ones do
int exblas_exspmv_csr_lp(int m, int n, int index_bits, const void *row_ptr, const void *col_idx, int val_dtype,
                         const void *val, double alpha, int vec_dtype, const void *x, double beta, void *y, int fpe,
                         int early_exit)
{
    if (int rc = csr_lp_precheck(m, n, 1, index_bits, row_ptr, val_dtype, val, vec_dtype, x, 1, y, 1, fpe)) return rc;
    return csr_host_call(
        "exblas_exspmv_csr_lp", m, n, 1, index_bits, row_ptr, col_idx, val, x, 1, y, 1, fpe,
        [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *d_x, double *d_y) {
            return exspmv_lp_on(c, m, n, index_bits, d_rp, d_ci, val_dtype, d_val, alpha, vec_dtype, d_x, beta, d_y, fpe,
                                early_exit, c.stream);
        },
        0, (size_t)dtype_bytes(val_dtype), (size_t)dtype_bytes(vec_dtype));
}

int exblas_exspmm_csr_lp(int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx, int val_dtype,
                         const void *val, double alpha, int vec_dtype, const void *x, int64_t ldx, double beta, void *y,
                         int64_t ldy, int fpe, int early_exit)
{
    if (int rc = csr_lp_precheck(m, n, k, index_bits, row_ptr, val_dtype, val, vec_dtype, x, ldx, y, ldy, fpe)) return rc;
    return csr_host_call(
        "exblas_exspmm_csr_lp", m, n, k, index_bits, row_ptr, col_idx, val, x, ldx, y, ldy, fpe,
        [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *d_x, double *d_y) {
            return exspmm_lp_on(c, m, n, k, index_bits, d_rp, d_ci, val_dtype, d_val, alpha, vec_dtype, d_x, ldx, beta, d_y,
                                ldy, fpe, early_exit, c.stream);
        },
        0, (size_t)dtype_bytes(val_dtype), (size_t)dtype_bytes(vec_dtype));
}

// the shared CSR host path with no X: x (b on entry, the solution on return) travels as its Y
int exblas_exsptrsv_csr(char uplo, char diag, int m, int index_bits, const void *row_ptr, const void *col_idx,
                        const double *val, double *x, int fpe, int early_exit)
{
    if (!one_of(uplo, "LlUu") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    const int rc = csr_host_call("exblas_exsptrsv_csr", m, 0, 1, index_bits, row_ptr, col_idx, val, nullptr, 1, x, 1, fpe,
                                 [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *, double *d_x) {
                                     return exsptrsv_on(c, uplo, diag, m, index_bits, d_rp, d_ci, d_val, d_x, fpe, early_exit,
                                                        c.stream);
                                 });
    return (rc || m == 0) ? rc : host_solve_status(&CtxWsPtrs::sptrsv_info_dev);
}

int exblas_exspilu0_csr(int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val, double *lu,
                        int64_t *info, int fpe, int early_exit)
{
    return csr_factor_host("exblas_exspilu0_csr", &CtxWsPtrs::spilu0_info_dev, m, index_bits, row_ptr, col_idx, val, lu, info,
                           fpe, [&](Ctx &c, int m_, int ib, const void *rp, const void *ci, const double *v, double *y,
                                    int64_t *inf, hipStream_t st) {
                               return exspilu0_on(c, m_, ib, rp, ci, v, y, inf, fpe, early_exit, st);
                           });
}

int exblas_exspic0_csr(int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val, double *ll,
                       int64_t *info, int fpe, int early_exit)
{
    return csr_factor_host("exblas_exspic0_csr", &CtxWsPtrs::spic0_info_dev, m, index_bits, row_ptr, col_idx, val, ll, info,
                           fpe, [&](Ctx &c, int m_, int ib, const void *rp, const void *ci, const double *v, double *y,
                                    int64_t *inf, hipStream_t st) {
                               return exspic0_on(c, m_, ib, rp, ci, v, y, inf, fpe, early_exit, st);
                           });
}

// the same with a block: X (m x k, row stride ldx; B on entry, the solution on return) travels as the host path's Y
int exblas_exsptrsm_csr(char uplo, char diag, int m, int k, int index_bits, const void *row_ptr, const void *col_idx,
                        const double *val, double *x, int64_t ldx, int fpe, int early_exit)
{
    if (!one_of(uplo, "LlUu") || !one_of(diag, "NnUu")) return (int)hipErrorInvalidValue;
    const int rc = csr_host_call("exblas_exsptrsm_csr", m, 0, k, index_bits, row_ptr, col_idx, val, nullptr, k, x, ldx, fpe,
                                 [&](Ctx &c, const void *d_rp, const void *d_ci, const double *d_val, const double *, double *d_x) {
                                     return exsptrsm_on(c, uplo, diag, m, k, index_bits, d_rp, d_ci, d_val, d_x, ldx, fpe,
                                                        early_exit, c.stream);
                                 });
    return (rc || m == 0 || k == 0) ? rc : host_solve_status(&CtxWsPtrs::sptrsm_info_dev);
}

// the n columns of A travel with their lda padding (the last one only up to its n-th entry), and whole rows of X (the
// last one only up to its k-th entry), which come back the same way: the padding of X returns as it went
int exblas_extrsm(char uplo, char transa, char diag, int n, int k, const double *a, int lda, double *x, int64_t ldx,
                  int fpe, int early_exit)
{
    bool empty;
    const int bad = trsm_check_args(uplo, transa, diag, n, k, a, lda, x, ldx, fpe, &empty);
    if (bad || empty) return bad;
    {
        HostCall hc("exblas_extrsm");
        const size_t abytes = ((size_t)lda * (size_t)(n - 1) + (size_t)n) * sizeof(double);
        const size_t xbytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)k) * sizeof(double);
        double *d_a = hc.in(0, abytes, a, abytes);
        double *d_x = hc.in(1, xbytes, x, xbytes);
        hc.out(extrsm_on(hc.c, uplo, transa, diag, n, k, d_a, lda, d_x, ldx, fpe, early_exit, hc.c.stream), x, d_x, xbytes);
    }
    return host_solve_status(&CtxWsPtrs::trsm_info_dev);
}

// whole rows travel, padding included (the last row only up to its last entry); C comes back the same way, so that its
// padding returns as it went
int exblas_exbdot(char mode, int64_t n, int p, int q, const double *x, int64_t ldx, const double *y, int64_t ldy,
                  double *cm, int64_t ldc, int fpe, int early_exit)
{
    bool empty;
    const int bad = bdot_check_args(mode, n, p, q, x, ldx, y, ldy, cm, ldc, fpe, &empty);
    if (bad || empty) return bad;
    const bool diag = mode == 'D' || mode == 'd';
    HostCall hc("exblas_exbdot");
    const size_t xspan = n > 0 ? (size_t)(n - 1) * (size_t)ldx + (size_t)p : 0;
    const size_t yspan = n > 0 ? (size_t)(n - 1) * (size_t)ldy + (size_t)q : 0;
    const size_t cspan = diag ? (size_t)p : (size_t)(p - 1) * (size_t)ldc + (size_t)q;
    double *d_x = hc.in(0, xspan * 8 + 8, x, xspan * 8);
    double *d_y = hc.in(1, yspan * 8 + 8, y, yspan * 8);
    double *d_c = hc.in(2, cspan * 8, cm, cspan * 8);
    return hc.out(exbdot_on(hc.c, mode, n, p, q, d_x, ldx, d_y, ldy, d_c, ldc, fpe, early_exit, hc.c.stream), cm, d_c,
                  cspan * 8);
}

// whole rows of X, C and Y travel, padding included (the last row of each only up to its last entry); Y comes back the
// same way, so that its padding returns as it went
int exblas_exbgemm(int64_t n, int p, int q, double alpha, const double *x, int64_t ldx, const double *cm, int64_t ldc,
                   double beta, double *y, int64_t ldy, int fpe, int early_exit)
{
    bool empty;
    const int bad = bgemm_check_args(n, p, q, x, ldx, cm, ldc, y, ldy, fpe, &empty);
    if (bad || empty) return bad;
    HostCall hc("exblas_exbgemm");
    const size_t xspan = p > 0 ? (size_t)(n - 1) * (size_t)ldx + (size_t)p : 0;
    const size_t cspan = p > 0 ? (size_t)(p - 1) * (size_t)ldc + (size_t)q : 0;
    const size_t yspan = (size_t)(n - 1) * (size_t)ldy + (size_t)q;
    double *d_x = hc.in(0, xspan * 8 + 8, x, xspan * 8);
    double *d_c = hc.in(1, cspan * 8 + 8, cm, cspan * 8);
    double *d_y = hc.in(2, yspan * 8, y, yspan * 8);
    return hc.out(exbgemm_on(hc.c, n, p, q, alpha, d_x, ldx, d_c, ldc, beta, d_y, ldy, fpe, early_exit, hc.c.stream), y, d_y,
                  yspan * 8);
}

// the p columns of T travel with their ldt padding (the last one only up to its p-th entry), and whole rows of X (the
// last one only up to its p-th entry), which come back the same way: the padding of X returns as it went
int exblas_exbtrsm(char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *t, int ldt, double *x,
                   int64_t ldx, int fpe, int early_exit)
{
    bool empty;
    const int bad = btrsm_check_args(uplo, transt, diag, n, p, t, ldt, x, ldx, fpe, &empty);
    if (bad || empty) return bad;
    HostCall hc("exblas_exbtrsm");
    const size_t tbytes = ((size_t)ldt * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    const size_t xbytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)p) * sizeof(double);
    double *d_t = hc.in(0, tbytes, t, tbytes);
    double *d_x = hc.in(1, xbytes, x, xbytes);
    return hc.out(exbtrsm_on(hc.c, uplo, transt, diag, n, p, alpha, d_t, ldt, d_x, ldx, fpe, early_exit, hc.c.stream), x, d_x,
                  xbytes);
}

// the p columns of G travel with their ldg padding (the last one only up to its p-th entry) and come back the same way;
// *info (when given) receives the info word
int exblas_expotrf(char uplo, int p, double *g, int ldg, int *info, int fpe, int early_exit)
{
    bool empty;
    int dummy = 0;
    const int bad = potrf_check_args(uplo, p, g, ldg, &dummy, fpe, &empty);
    if (bad || empty) return bad;   // (p == 0: *info is not written either)
    HostCall hc("exblas_expotrf");
    const size_t gbytes = ((size_t)ldg * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    double *d_g = hc.in(0, gbytes, g, gbytes);
    int *d_info = (int *)hc.in(1, sizeof(int), nullptr, 0);
    const int rc = expotrf_on(hc.c, uplo, p, d_g, ldg, d_info, fpe, early_exit, hc.c.stream);
    if (rc == 0 && info) EXB_CHECK(hipMemcpyAsync(info, d_info, sizeof(int), hipMemcpyDeviceToHost, hc.c.stream));
    return hc.out(rc, g, d_g, gbytes);
}

// the matrices travel as one span, from the first entry of the first to the p-th entry of the last column of the last
// (padding, gaps and the other triangles included), and come back the same way; info (when given) receives the batch words
int exblas_expotrf_batched(char uplo, int p, int64_t batch, double *g, int ldg, int64_t stride, int *info, int fpe,
                           int early_exit)
{
    bool empty;
    int dummy = 0;
    const int bad = potrf_batched_check_args(uplo, p, batch, g, ldg, stride, &dummy, fpe, &empty);
    if (bad || empty) return bad;   // (nothing to do: info is not written either)
    HostCall hc("exblas_expotrf_batched");
    const size_t gbytes = ((size_t)(batch - 1) * (size_t)stride + (size_t)ldg * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    const size_t ibytes = (size_t)batch * sizeof(int);
    double *d_g = hc.in(0, gbytes, g, gbytes);
    int *d_info = (int *)hc.in(1, ibytes, nullptr, 0);
    const int rc = expotrf_batched_on(hc.c, uplo, p, batch, d_g, ldg, stride, d_info, fpe, early_exit, hc.c.stream);
    if (rc == 0 && info) EXB_CHECK(hipMemcpyAsync(info, d_info, ibytes, hipMemcpyDeviceToHost, hc.c.stream));
    return hc.out(rc, g, d_g, gbytes);
}

// the triangles travel as one span (as above), and whole rows of X (the last one only up to its k-th entry), which come
// back the same way: the padding of X returns as it went
int exblas_expotrs_batched(char uplo, char sweep, int p, int64_t n, int k, const double *r, int ldr, int64_t stride, double *x,
                           int64_t ldx, int fpe, int early_exit)
{
    bool empty;
    const int bad = potrs_batched_check_args(uplo, sweep, p, n, k, r, ldr, stride, x, ldx, fpe, &empty);
    if (bad || empty) return bad;
    HostCall hc("exblas_expotrs_batched");
    const size_t nblocks = (size_t)((n + p - 1) / p);
    const size_t rbytes = ((nblocks - 1) * (size_t)stride + (size_t)ldr * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    const size_t xbytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)k) * sizeof(double);
    double *d_r = hc.in(0, rbytes, r, rbytes);
    double *d_x = hc.in(1, xbytes, x, xbytes);
    return hc.out(expotrs_batched_on(hc.c, uplo, sweep, p, n, k, d_r, ldr, stride, d_x, ldx, fpe, early_exit, hc.c.stream), x,
                  d_x, xbytes);
}

// the matrices travel as one span, from the first entry of the first to the last entry of the last (padding and gaps
// included), and come back the same way; ipiv and info (when given) receive the batch * p pivots and the batch words
int exblas_exgetrf_batched(char order, int p, int64_t batch, double *a, int lda, int64_t stride, int *ipiv, int *info, int fpe,
                           int early_exit)
{
    bool empty;
    int dummy = 0;
    const int bad = getrf_batched_check_args(order, p, batch, a, lda, stride, &dummy, &dummy, fpe, &empty);
    if (bad || empty) return bad;   // (nothing to do: ipiv and info are not written either)
    HostCall hc("exblas_exgetrf_batched");
    const size_t abytes = ((size_t)(batch - 1) * (size_t)stride + (size_t)lda * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    const size_t ibytes = (size_t)batch * sizeof(int), pbytes = ibytes * (size_t)p;
    double *d_a = hc.in(0, abytes, a, abytes);
    int *d_info = (int *)hc.in(1, ibytes, nullptr, 0);
    int *d_ipiv = (int *)hc.in(2, pbytes, nullptr, 0);
    const int rc = exgetrf_batched_on(hc.c, order, p, batch, d_a, lda, stride, d_ipiv, d_info, fpe, early_exit, hc.c.stream);
    if (rc == 0 && info) EXB_CHECK(hipMemcpyAsync(info, d_info, ibytes, hipMemcpyDeviceToHost, hc.c.stream));
    if (rc == 0 && ipiv) EXB_CHECK(hipMemcpyAsync(ipiv, d_ipiv, pbytes, hipMemcpyDeviceToHost, hc.c.stream));
    return hc.out(rc, a, d_a, abytes);
}

// the factors travel as one span (as above) with their pivots, and whole rows of X (the last one only up to its k-th
// entry), which come back the same way: the padding of X returns as it went
int exblas_exgetrs_batched(char order, int p, int64_t n, int k, const double *lu, int ldlu, int64_t stride, const int *ipiv,
                           double *x, int64_t ldx, int fpe, int early_exit)
{
    bool empty;
    const int bad = getrs_batched_check_args(order, p, n, k, lu, ldlu, stride, ipiv, x, ldx, fpe, &empty);
    if (bad || empty) return bad;
    HostCall hc("exblas_exgetrs_batched");
    const size_t nblocks = (size_t)((n + p - 1) / p);
    const size_t lbytes = ((nblocks - 1) * (size_t)stride + (size_t)ldlu * (size_t)(p - 1) + (size_t)p) * sizeof(double);
    const size_t pbytes = nblocks * (size_t)p * sizeof(int);
    const size_t xbytes = ((size_t)(n - 1) * (size_t)ldx + (size_t)k) * sizeof(double);
    double *d_lu = hc.in(0, lbytes, lu, lbytes);
    double *d_x = hc.in(1, xbytes, x, xbytes);
    const int *d_ipiv = (const int *)hc.in(2, pbytes, ipiv, pbytes);
    return hc.out(exgetrs_batched_on(hc.c, order, p, n, k, d_lu, ldlu, stride, d_ipiv, d_x, ldx, fpe, early_exit, hc.c.stream),
                  x, d_x, xbytes);
}

int exblas_exgemm(char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                  const double *b, int ldb, double beta, double *cm, int ldc, int fpe, int early_exit)
{
    check_fpe(fpe);
    if (m <= 0 || n <= 0) return 0;
    HostCall hc("exblas_exgemm");
    const bool ta = (transa == 'T' || transa == 't'), tb = (transb == 'T' || transb == 't');
    // row-major storage (ExGEMM.Superacc.cl:254-255): A is m x k (k x m when transposed), etc.
    const size_t abytes = (size_t)(ta ? k : m) * (size_t)lda * sizeof(double);
    const size_t bbytes = (size_t)(tb ? n : k) * (size_t)ldb * sizeof(double);
    const size_t cbytes = (size_t)m * (size_t)ldc * sizeof(double);
    double *d_a = hc.in(0, abytes, a, abytes);
    double *d_b = hc.in(1, bbytes, b, bbytes);
    double *d_c = hc.in(2, cbytes, cm, cbytes);
    return hc.out(exgemm_on(hc.c, transa, transb, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, fpe, early_exit,
                            hc.c.stream),
                  cm, d_c, cbytes);
}

}  // extern "C"

// =============================================================================================
// C++ API with the reference's signatures (global namespace, C++ linkage)
// =============================================================================================
double exsum(const int Ng, double *ag, const int inca, const int offset, const int fpe, const bool early_exit,
             const bool parallel)
{
    (void)parallel;  // "Does not affect GPU implementation since it is always parallel" (gpu:ExSUM.cpp:61)
    return exblas_exsum(Ng, ag, inca, offset, fpe, early_exit ? 1 : 0);
}

double exdot(const int Ng, double *ag, const int inca, const int offseta, double *bg, const int incb,
             const int offsetb, const int fpe, const bool early_exit)
{
    return exblas_exdot(Ng, ag, inca, offseta, bg, incb, offsetb, fpe, early_exit ? 1 : 0);
}

int exgemv(const char transa, const int m, const int n, const double alpha, double *a, const int lda,
           const int offseta, double *x, const int incx, const int offsetx, const double beta, double *y,
           const int incy, const int offsety, const int fpe, const bool early_exit)
{
    return exblas_exgemv(transa, m, n, alpha, a, lda, offseta, x, incx, offsetx, beta, y, incy, offsety, fpe,
                         early_exit ? 1 : 0);
}

int extrsv(const char uplo, const char transa, const char diag, const int n, double *a, const int lda,
           const int offseta, double *x, const int incx, const int offsetx, const int fpe, const bool early_exit)
{
    return exblas_extrsv(uplo, transa, diag, n, a, lda, offseta, x, incx, offsetx, fpe, early_exit ? 1 : 0);
}

int exgemm(char transa, char transb, int m, int n, int k, double alpha, double *a, int lda, double *b, int ldb,
           double beta, double *c, int ldc, int fpe, bool early_exit)
{
    return exblas_exgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, fpe, early_exit ? 1 : 0);
}
