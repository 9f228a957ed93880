// extern "C" boundary of libgpfq_hip.so (declared in include/gpfq.h).  Argument validation,
// path selection and error reporting; no allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/gpfq.h"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"

namespace {

thread_local char g_err[512] = "";
thread_local const char *g_dense_kernel = "";
thread_local hipEvent_t g_main_ev[2] = {nullptr, nullptr};

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(GPFQ_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

// The host alphabet as the by-value kernel arguments: A for up to 64 members (int8 indices, every kernel family), B beyond
// (65..GPFQ_MAX_ALPHABET members, int16 indices: the wavefront-per-neuron, wide, streaming and thread-per-neuron Gram kernels).
struct HostAlphabet {
    gpfq::AlphabetArg A;
    gpfq::AlphabetBig B;
    bool is_big = false;
    const gpfq::AlphabetBig *big() const { return is_big ? &B : nullptr; }
    size_t idx_bytes() const { return is_big ? 2 : 1; }
    // element offset into an index array of either width
    int8_t *at(void *qidx, int64_t elems) const { return qidx ? static_cast<int8_t *>(qidx) + elems * (int64_t)idx_bytes() : nullptr; }
};

// Copies the host alphabet into the kernel argument of its size class and classifies it.
int make_alphabet(const double *alphabet, int M, int zero_idx, HostAlphabet *H)
{
    if (!alphabet) return fail(GPFQ_ERR_INVALID_ARG, "alphabet is NULL");
    if (M < 1) return fail(GPFQ_ERR_INVALID_ARG, "alphabet size M=%d must be >= 1", M);
    if (M > GPFQ_MAX_ALPHABET)
        return fail(GPFQ_ERR_UNSUPPORTED, "alphabet size M=%d exceeds GPFQ_MAX_ALPHABET=%d", M, GPFQ_MAX_ALPHABET);
    if (zero_idx < -1 || zero_idx >= M) return fail(GPFQ_ERR_INVALID_ARG, "zero_idx=%d out of range", zero_idx);
    std::memset(&H->A, 0, sizeof(H->A));
    std::memset(&H->B, 0, sizeof(H->B));
    H->is_big = M > 64;
    bool asc = true;
    for (int k = 0; k < M; ++k) {
        if (H->is_big) H->B.a[k] = alphabet[k];
        else H->A.a[k] = alphabet[k];
        if (std::isnan(alphabet[k])) asc = false;
        if (k > 0 && !(alphabet[k - 1] <= alphabet[k])) asc = false;
    }
    H->A.M = H->B.M = M;
    H->A.zero_idx = H->B.zero_idx = zero_idx;
    H->A.ascending = H->B.ascending = asc ? 1 : 0;
    return GPFQ_OK;
}

// The options (gpfq_options.hpp): the table's rows, and the process-wide store -- one relaxed atomic per row, in the table's order.
struct OptionRow {
    const char *key;
    int gpfq::Options::*member;
    bool (*accepts)(int);
    int (*stores)(int);
    const char *domain;
};
#define GPFQ_OPTION_ROW(key, def, accepts, stores, domain) \
    {#key, &gpfq::Options::key, [](int v) { (void)v; return (bool)(accepts); }, [](int v) { return (int)(stores); }, domain},
const OptionRow kOptionRows[] = {GPFQ_OPTIONS(GPFQ_OPTION_ROW)};
#undef GPFQ_OPTION_ROW
#define GPFQ_OPTION_DEFAULT(key, def, accepts, stores, domain) {def},
std::atomic<int> option_store[] = {GPFQ_OPTIONS(GPFQ_OPTION_DEFAULT)};
#undef GPFQ_OPTION_DEFAULT
constexpr int kOptionCount = (int)(sizeof(kOptionRows) / sizeof(kOptionRows[0]));

int option_index(const char *key)
{
    for (int i = 0; i < kOptionCount; ++i)
        if (!std::strcmp(key, kOptionRows[i].key)) return i;
    return -1;
}

}  // namespace

namespace gpfq {
Options options_snapshot()
{
    Options o;
    for (int i = 0; i < kOptionCount; ++i) o.*kOptionRows[i].member = option_store[i].load(std::memory_order_relaxed);
    return o;
}
void note_dense_kernel(const char *name) { g_dense_kernel = name; }
bool main_kernel_events(hipEvent_t *start, hipEvent_t *stop)
{
    *start = g_main_ev[0]; *stop = g_main_ev[1];
    return g_main_ev[0] != nullptr && g_main_ev[1] != nullptr;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): it is raised when a launch needs more than
// any launch before it on that device, not once per launch.
hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = granted[std::make_pair(kernel, dev)];
    if (bytes <= have) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}
}

extern "C" {

int gpfq_version(void) { return 306; }   // 306: the two-pass median's workspace grew by its coarse histograms (gpfq_median_abs_workspace_bytes_for), gpfq_set_main_kernel_events' events ride on the kernel's dispatch, option blk_prep_norms (round 6); 305: device-resident layer alphabet, gpfq_quantize_dense_layer, gpfq_call_status, the block kernel's workspace grew by its alphabet block (round 6); 304: options blk_cluster / blk_cluster_nl / blk_cluster_map, larger workspaces for long rows (round 5); 303: gpfq_set_main_kernel_events (round 4); hip.load() checks it

const char *gpfq_last_dense_kernel(void) { return g_dense_kernel; }

int gpfq_set_main_kernel_events(void *start, void *stop)
{
    g_main_ev[0] = static_cast<hipEvent_t>(start);
    g_main_ev[1] = static_cast<hipEvent_t>(stop);
    return GPFQ_OK;
}

const char *gpfq_last_error(void) { return g_err; }

int gpfq_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

int gpfq_row_norms(const float *Xq, int64_t N, int64_t m, int64_t ld, float *nrm32, void *stream)
{
    if (N < 0 || m < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld m=%lld", (long long)N, (long long)m);
    if (N == 0) return GPFQ_OK;
    if (!nrm32 || (!Xq && m > 0)) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < m=%lld", (long long)ld, (long long)m);
    hipError_t e = gpfq::launch_row_norms(Xq, N, m, ld, nrm32, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_row_norms");
}

static int resolve_path(int64_t m, int path)
{
    if (path == GPFQ_PATH_AUTO) return m <= GPFQ_ONCHIP_MAX_M ? GPFQ_PATH_ONCHIP : GPFQ_PATH_STREAM;
    return path;
}

// GPFQ_PATH_AUTO prefers the Gram path (N x N records + scalar recurrences, gpfq_quantize_neurons_gram) exactly where
// the Python binding's auto_path does: rows beyond GPFQ_GRAM_MIN_M samples (or half of that with many neurons), walks
// the records can hold, and no residual vectors requested.
static bool auto_wants_gram(int64_t N, int64_t m, int64_t C, bool want_u)
{
    const bool long_rows = m > GPFQ_GRAM_MIN_M || (m > GPFQ_GRAM_MIN_M / 2 && C * m >= 5000000);
    return !want_u && long_rows && N <= GPFQ_GRAM_MAX_N && m < (1LL << 30);
}

// on-chip workspace: [fallback counter, 64 B][RowStats x N][iteration records of the pipelined kernel]
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t onchip_stats_bytes(int64_t N) { return al256(64 + (size_t)N * sizeof(gpfq::RowStats)); }
static size_t onchip_workspace_bytes(int64_t N, int64_t m, int64_t C, const gpfq::Options &o)
{
    const size_t p = gpfq::pipe_workspace_bytes(N, m), b = gpfq::blk_workspace_bytes(N, m, C, o);
    return onchip_stats_bytes(N) + (p > b ? p : b);
}

// AUTO -> Gram: [Gram workspace][uncertified flags i32 x C][streaming workspace of ONE neuron, for the rare reruns]
static size_t auto_gram_workspace_bytes(int64_t N, int64_t m, int64_t C)
{
    return al256(gpfq::gram_workspace_bytes(N, m, C)) + al256((size_t)C * sizeof(int32_t)) +
           gpfq::stream_workspace_bytes(N, m, 1, /*need_u=*/true);
}

size_t gpfq_workspace_bytes(int64_t N, int64_t m, int64_t C, int path)
{
    if (N < 0 || m < 0 || C < 0) return 0;
    const gpfq::Options o = gpfq::options_snapshot();
    size_t need = resolve_path(m, path) == GPFQ_PATH_ONCHIP ? onchip_workspace_bytes(N, m, C, o)
                                                             : gpfq::stream_workspace_bytes(N, m, C, /*need_u=*/true);
    if (path == GPFQ_PATH_AUTO && auto_wants_gram(N, m, C, false)) {
        const size_t g = auto_gram_workspace_bytes(N, m, C);
        if (g > need) need = g;
    }
    return need;
}

int gpfq_set_option(const char *key, int value)
{
    if (!key) return fail(GPFQ_ERR_INVALID_ARG, "option key is NULL");
    const int i = option_index(key);
    if (i < 0) return fail(GPFQ_ERR_INVALID_ARG, "unknown option '%s'", key);
    if (!kOptionRows[i].accepts(value)) return fail(GPFQ_ERR_INVALID_ARG, "%s must be %s", key, kOptionRows[i].domain);
    option_store[i].store(kOptionRows[i].stores(value), std::memory_order_relaxed);
    return GPFQ_OK;
}

int gpfq_get_option(const char *key, int *value)
{
    if (!key) return fail(GPFQ_ERR_INVALID_ARG, "option key is NULL");
    const int i = option_index(key);
    if (i < 0) return fail(GPFQ_ERR_INVALID_ARG, "unknown option '%s'", key);
    if (!value) return fail(GPFQ_ERR_INVALID_ARG, "option '%s': value is NULL", key);
    *value = option_store[i].load(std::memory_order_relaxed);
    return GPFQ_OK;
}

int gpfq_call_status(const void *workspace, void *stream)
{
    if (!workspace) return fail(GPFQ_ERR_INVALID_ARG, "workspace is NULL");
    // (a pinned landing buffer per calling thread, allocated at the first use and kept: a 16-byte copy into pageable memory goes through
    //  the runtime's staging path and cost a 0.15 ms layer 0.05 ms)
    static thread_local int32_t *pinned = nullptr;
    int32_t stack_words[4] = {0, 0, 0, 0};
    if (!pinned && hipHostMalloc(reinterpret_cast<void **>(&pinned), 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pinned = nullptr; }
    int32_t *w = pinned ? pinned : stack_words;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(w, workspace, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "gpfq_call_status");
    if (w[2] != 0)
        return fail(GPFQ_ERR_CLUSTER_TIMEOUT, "an exchange between the workgroups of the block kernel's cluster form timed out (a slice never arrived): "
                                              "the outputs of this call are invalid; rerun it with gpfq_set_option(\"blk_cluster\", 0)");
    if (w[3] != 0)
        return fail(GPFQ_ERR_ALPHABET, "the device-resident alphabet is not a strictly ascending arithmetic progression (radius zero, infinite or NaN): "
                                       "nothing was computed; rerun the layer through gpfq_quantize_neurons with a host alphabet");
    return GPFQ_OK;
}

int gpfq_quantize_neurons(const float *X, const float *Xq, int64_t ld, const float *nrm32,
                          const float *Wt, int64_t ldw,
                          const double *alphabet, int M, int zero_idx,
                          int64_t N, int64_t m, int64_t C,
                          void *qidx_v, float *Qt, double *resid, double *u_out,
                          void *workspace, size_t workspace_bytes, int path, void *stream)
{
    if (N < 0 || m < 0 || C < 0)
        return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld m=%lld C=%lld", (long long)N, (long long)m, (long long)C);
    HostAlphabet H;
    int rc = make_alphabet(alphabet, M, zero_idx, &H);
    if (rc != GPFQ_OK) return rc;
    const gpfq::AlphabetArg &A = H.A;
    int8_t *qidx = static_cast<int8_t *>(qidx_v);          // int16 elements when H.is_big
    if (C == 0) return GPFQ_OK;
    if (N > 0 && (!Wt || !nrm32)) return fail(GPFQ_ERR_INVALID_ARG, "Wt/nrm32 is NULL");
    if (N > 0 && m > 0 && (!X || !Xq)) return fail(GPFQ_ERR_INVALID_ARG, "X/Xq is NULL");
    if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < m=%lld", (long long)ld, (long long)m);
    if (ldw < N) return fail(GPFQ_ERR_INVALID_ARG, "weight pitch ldw=%lld < N=%lld", (long long)ldw, (long long)N);
    if (path != GPFQ_PATH_AUTO && path != GPFQ_PATH_ONCHIP && path != GPFQ_PATH_STREAM)
        return fail(GPFQ_ERR_INVALID_ARG, "unknown path %d", path);
    const int p = resolve_path(m, path);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const gpfq::Options o = gpfq::options_snapshot();

    // (alphabets beyond 64 members have no wavefront-per-neuron chain for walks beyond 64 steps: those stay on the element-wise paths)
    if (path == GPFQ_PATH_AUTO && o.auto_gram && N > 0 && m > 0 && auto_wants_gram(N, m, C, u_out != nullptr) && !(H.is_big && N > 64) && workspace &&
        (uintptr_t)workspace % 16 == 0 && workspace_bytes >= auto_gram_workspace_bytes(N, m, C)) {
        // Long rows, short walks: Gram records once per layer, the recurrence on scalars with every decision certified,
        // uncertifiable chains repaired on the device; whatever is still flagged afterwards (practically never) is rerun
        // here through the streaming kernel, which costs this call ONE stream synchronisation (the flags cross to the host).
        char *ws = static_cast<char *>(workspace);
        void *gram_ws = ws;
        int32_t *unc = reinterpret_cast<int32_t *>(ws + al256(gpfq::gram_workspace_bytes(N, m, C)));
        char *stream_ws = reinterpret_cast<char *>(unc) + al256((size_t)C * sizeof(int32_t));
        gpfq::GramArgs g;
        g.X = X; g.Xq = Xq; g.ld = ld; g.nrm32 = nrm32; g.Wt = Wt; g.ldw = ldw; g.A = A; g.big = H.big();
        g.N = N; g.m = m; g.C = C; g.qidx = qidx; g.Qt = Qt; g.resid = resid; g.uncertified = unc;
        g.workspace = gram_ws;
        g.slack = std::ldexp(1.0, o.gram_slack_log2);
        g.opt = o;
        gpfq::note_dense_kernel("gpfq_gram_* (Gram records + certified scalar recurrence), reruns through gpfq_stream_*");
        hipError_t e = gpfq::launch_gram(g, s);
        if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_neurons(auto: gram)");
        std::vector<int32_t> flags((size_t)C);
        e = hipMemcpyAsync(flags.data(), unc, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_neurons(auto: flags)");
        for (int64_t j = 0; j < C; ++j) {
            if (!flags[(size_t)j]) continue;
            gpfq::StreamArgs a;
            a.X = X; a.Xq = Xq; a.ld = ld; a.nrm32 = nrm32; a.Wt = Wt + j * ldw; a.ldw = ldw; a.A = A; a.big = H.big();
            a.N = N; a.m = m; a.C = 1; a.qidx = H.at(qidx, j * N); a.Qt = Qt ? Qt + j * N : nullptr;
            a.resid = resid ? resid + j : nullptr; a.u_out = nullptr;
            a.workspace = stream_ws; a.workspace_bytes = gpfq::stream_workspace_bytes(N, m, 1, true);
            e = gpfq::launch_stream(a, s);
            if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_neurons(auto: rerun)");
        }
        return GPFQ_OK;
    }

    if (p == GPFQ_PATH_ONCHIP) {
        if (m > GPFQ_ONCHIP_MAX_M)
            return fail(GPFQ_ERR_UNSUPPORTED, "on-chip path needs m <= %d (got %lld)", GPFQ_ONCHIP_MAX_M, (long long)m);
        gpfq::OnchipArgs a;
        a.X = X; a.Xq = Xq; a.ld = ld; a.nrm32 = nrm32; a.Wt = Wt; a.ldw = ldw; a.A = A; a.big = H.big();
        a.N = N; a.m = m; a.C = C; a.qidx = qidx; a.Qt = Qt; a.resid = resid; a.u_out = u_out;
        a.mode = o.onchip_mode;
        a.opt = o;
        // certified mode needs the per-row statistics in the workspace; without one, run the exact flow
        const bool have_ws = workspace && workspace_bytes >= onchip_stats_bytes(N) && (uintptr_t)workspace % 16 == 0;
        bool counters_zeroed = false;
        auto zero_counters = [&]() -> hipError_t {             // the call's counter block: exact fallbacks, cluster timeout, alphabet word
            if (!have_ws || counters_zeroed) return hipSuccess;
            counters_zeroed = true;
            return hipMemsetAsync(workspace, 0, 64, s);
        };
        // the pipelined kernel (gpfq_pipe.hip): rows of up to 2048 samples in layers wide enough to fill the chip
        // with 16 neurons per workgroup; narrow layers keep the latency-oriented kernels below
        if (!H.is_big) {
            gpfq::PipeArgs pa;
            pa.X = X; pa.Xq = Xq; pa.ld = ld; pa.nrm32 = nrm32; pa.Wt = Wt; pa.ldw = ldw; pa.A = A;
            pa.N = N; pa.m = m; pa.C = C; pa.qidx = qidx; pa.Qt = Qt; pa.resid = resid; pa.u_out = u_out;
            pa.opt = o;
            const bool forced_old = o.lanes_per_neuron != 0 || o.waves_per_neuron != 0 || o.onchip_mode != 1 || o.pipe == 0;
            // measured (tools/blk_ab.sh shapes): the block-pipelined kernel is ahead of the row-group and wavefront-per-neuron kernels
            // for rows of 257..4096 samples (2049+: one step per slot; 4096 x 4096 x 4096: 16.6 vs 38 ms) whenever the layer has 512 neurons or more (4096 x 4096, m = 1024: 4.1 vs 5.4 ms;
            // m = 2048, 16 levels: 8.7 vs 10.0; m = 512: 3.2 vs 3.9; 4096 x 1024, m = 1536: 3.7 vs 6.8; 784 x 4096, m = 512: 0.68
            // vs 0.85).  Its time per step does not depend on the number of neurons up to one workgroup per CU; narrower layers
            // stay with the kernels that split a neuron over several wavefronts (4096 x 128, m = 512: 3.05 vs 3.16 ms; m = 2048:
            // 2.06 vs 2.20) -- except for rows of 769+ samples, where workgroups of 8 and of 4 neurons make it the fastest at any
            // width (4096 x 2048, m = 1024: 2.5 vs 5.4 ms; 4096 x 128, m = 2048: 2.9 vs 4.5; 2048 x 128, m = 4096: 2.3 vs 2.5).
            // Round 3: two-neuron workgroups (layers of at most 512 neurons, rows of up to 5120 samples) make it the fastest for narrow
            // layers as well (784 x 128, m = 512, 16 levels; 2048 x 128, m = 5008: tools/blk_ab.sh latency, profiles/r03/).
            // Round 5: rows of 5121..28672 samples too -- the cluster form (gpfq_blk.hip: slices of 1024 samples over several workgroups;
            // blk_supported() says no when the option blk_cluster switches it off)
            const bool fits = m > 256 && M <= 64 && m <= GPFQ_ONCHIP_MAX_M;
            const bool want = o.pipe == 1;
            if ((o.pipe == 2 || (o.pipe < 0 && !forced_old && fits)) && N > 0 && m > 0 && gpfq::blk_supported(pa) && workspace &&
                (uintptr_t)workspace % 16 == 0 && workspace_bytes >= onchip_workspace_bytes(N, m, C, o)) {
                pa.workspace = static_cast<char *>(workspace) + onchip_stats_bytes(N);
                pa.fallback_count = static_cast<unsigned long long *>(workspace);
                pa.zero_counters = 1;                              // (the kernel that stores the alphabet zeroes the counter block as well: one launch, no memset)
                hipError_t e = gpfq::launch_blk(pa, s);             // (notes its kernel family itself, by the instantiation it resolves)
                if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_neurons(block-pipelined)");
                return o.sync_errors ? gpfq_call_status(workspace, stream) : GPFQ_OK;
            }
            if (want && N > 0 && m > 0 && gpfq::pipe_supported(pa) && workspace && (uintptr_t)workspace % 16 == 0 &&
                workspace_bytes >= onchip_workspace_bytes(N, m, C, o)) {
                hipError_t ez = zero_counters();
                if (ez != hipSuccess) return hip_fail(ez, "gpfq_quantize_neurons(workspace)");
                pa.workspace = static_cast<char *>(workspace) + onchip_stats_bytes(N);
                pa.fallback_count = static_cast<unsigned long long *>(workspace);
                gpfq::note_dense_kernel("gpfq_pipe_kernel (8 sweep wavefronts over the sample axis + 1 decision wavefront per workgroup)");
                hipError_t e = gpfq::launch_pipe(pa, s);
                return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_neurons(pipelined)");
            }
        }
        {
            hipError_t ez = zero_counters();
            if (ez != hipSuccess) return hip_fail(ez, "gpfq_quantize_neurons(workspace)");
        }
        if (a.mode == 1 && N > 0 && have_ws) {
            auto *stats = reinterpret_cast<gpfq::RowStats *>(static_cast<char *>(workspace) + 64);
            a.fallback_count = static_cast<unsigned long long *>(workspace);
            hipError_t e0 = gpfq::launch_row_stats(X, Xq, N, m, ld, nrm32, stats, s);
            if (e0 != hipSuccess) return hip_fail(e0, "gpfq_quantize_neurons(row stats)");
            a.stats = stats;
        } else {
            a.mode = 0;
        }
        hipError_t e = gpfq::launch_onchip(a, s);
        return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_neurons(on-chip)");
    }

    const size_t need = gpfq::stream_workspace_bytes(N, m, C, u_out == nullptr);
    if (!workspace || workspace_bytes < need)
        return fail(GPFQ_ERR_WORKSPACE, "streaming path needs %zu workspace bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    gpfq::StreamArgs a;
    a.X = X; a.Xq = Xq; a.ld = ld; a.nrm32 = nrm32; a.Wt = Wt; a.ldw = ldw; a.A = A; a.big = H.big();
    a.N = N; a.m = m; a.C = C; a.qidx = qidx; a.Qt = Qt; a.resid = resid; a.u_out = u_out;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    gpfq::note_dense_kernel("gpfq_stream_step_kernel + gpfq_stream_decide_kernel (residual in HBM)");
    hipError_t e = gpfq::launch_stream(a, s);
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_neurons(stream)");
}


// ---- the Dense layer driver as one call, alphabet in device memory (round 6) ----------------------------------------------------------
static int unit_alphabet_arg(const double *unit_alphabet, int M, HostAlphabet *H)
{
    if (!unit_alphabet) return fail(GPFQ_ERR_INVALID_ARG, "unit_alphabet is NULL");
    int zero_idx = -1;
    for (int k = 0; k < M && k < GPFQ_MAX_ALPHABET; ++k)
        if (unit_alphabet[k] == 0.0) zero_idx = k;
    return make_alphabet(unit_alphabet, M, zero_idx, H);
}

int gpfq_layer_alphabet_device(const float *median32, double alphabet_scalar, const double *unit_alphabet, int M,
                               void *dev_alphabet, void *stream)
{
    HostAlphabet H;
    int rc = unit_alphabet_arg(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    if (H.is_big) return fail(GPFQ_ERR_UNSUPPORTED, "device-resident alphabets hold up to 64 members (got %d)", M);
    if (!median32 || !dev_alphabet) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)dev_alphabet % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "dev_alphabet must be 16-byte aligned");
    hipError_t e = gpfq::launch_alphabet_device(median32, alphabet_scalar, H.A, dev_alphabet, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_layer_alphabet_device");
}

// Whether the alphabet gpfq_layer_alphabet_device would form from this median is one the block-pipelined kernel runs (DevAlphabet::ok):
// the same __host__ __device__ code on the host, no launch.  A caller that read the median back knows without the call's status.
int gpfq_device_alphabet_ok(float median32, double alphabet_scalar, const double *unit_alphabet, int M)
{
    HostAlphabet H;
    if (unit_alphabet_arg(unit_alphabet, M, &H) != GPFQ_OK || H.is_big) return 0;
    return gpfq::device_alphabet_of(median32, alphabet_scalar, H.A, gpfq::blk_unit_wants_sym(H.A) ? 1 : 0).ok;
}

// median(|W|) and the layer alphabet in one go: the last workgroup of the median's second pass forms the alphabet (no launch of its
// own between the two).  Needs the two-pass form: a 16-byte aligned kernel and gpfq_median_abs_workspace_bytes_for(n) of workspace.
int gpfq_layer_alphabet_from_kernel(const float *W, int64_t n, double alphabet_scalar, const double *unit_alphabet, int M,
                                    void *dev_alphabet, float *median_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n <= 0) return fail(GPFQ_ERR_INVALID_ARG, "median of %lld elements", (long long)n);
    HostAlphabet H;
    int rc = unit_alphabet_arg(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    if (H.is_big) return fail(GPFQ_ERR_UNSUPPORTED, "device-resident alphabets hold up to 64 members (got %d)", M);
    if (!W || !dev_alphabet) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)dev_alphabet % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "dev_alphabet must be 16-byte aligned");
    if ((uintptr_t)W % 16 != 0) return fail(GPFQ_ERR_UNSUPPORTED, "a kernel that is not 16-byte aligned: gpfq_median_abs + gpfq_layer_alphabet_device");
    if (!workspace || (uintptr_t)workspace % 16 != 0 || workspace_bytes < gpfq_median_abs_workspace_bytes_for(n))
        return fail(GPFQ_ERR_WORKSPACE, "gpfq_layer_alphabet_from_kernel needs %zu aligned workspace bytes", gpfq_median_abs_workspace_bytes_for(n));
    hipError_t e = gpfq::launch_median_abs(W, n, median_out, workspace, static_cast<hipStream_t>(stream), workspace_bytes,
                                           dev_alphabet, alphabet_scalar, &H.A, gpfq::blk_unit_wants_sym(H.A) ? 1 : 0);
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_layer_alphabet_from_kernel");
}

// The answers of gpfq_dense_layer_supported / _workspace_bytes under the caller's snapshot (dense_layer_impl: one call, one reading).
// *pa: what the block kernel's host-side queries are asked with.
static bool dense_layer_supported(int64_t N, int64_t m, int64_t C, const double *unit_alphabet, int M, const gpfq::Options &o, gpfq::PipeArgs *pa)
{
    if (N < 1 || m < 1 || C < 1 || !unit_alphabet || M < 1 || M > 64) return false;
    HostAlphabet H;
    if (unit_alphabet_arg(unit_alphabet, M, &H) != GPFQ_OK) return false;
    // exactly the rows and alphabets gpfq_quantize_neurons gives the block-pipelined kernel by default
    const bool forced_old = o.lanes_per_neuron != 0 || o.waves_per_neuron != 0 || o.onchip_mode != 1 || o.pipe == 0 || o.pipe == 1;
    if (forced_old || !(m > 256 && m <= GPFQ_ONCHIP_MAX_M)) return false;
    *pa = gpfq::PipeArgs{};
    pa->A = H.A; pa->N = N; pa->m = m; pa->C = C; pa->opt = o;
    return gpfq::blk_supported(*pa);
}

static size_t dense_layer_workspace_bytes(int64_t N, int64_t m, int64_t C, const gpfq::Options &o)
{
    if (N < 0 || m < 0 || C < 0) return 0;
    return onchip_workspace_bytes(N, m, C, o) + al256((size_t)N * sizeof(float));      // (+ the row norms when the caller passes none)
}

int gpfq_dense_layer_supported(int64_t N, int64_t m, int64_t C, const double *unit_alphabet, int M)
{
    gpfq::PipeArgs pa;
    return dense_layer_supported(N, m, C, unit_alphabet, M, gpfq::options_snapshot(), &pa) ? 1 : 0;
}

int gpfq_dense_layer_keras_out_supported(int64_t N, int64_t m, int64_t C, const double *unit_alphabet, int M)
{
    gpfq::PipeArgs pa;
    return dense_layer_supported(N, m, C, unit_alphabet, M, gpfq::options_snapshot(), &pa) && gpfq::blk_keras_out_supported(pa) ? 1 : 0;
}

int gpfq_blk_instance(int64_t N, int64_t m, int64_t C, const double *alphabet, int M, int32_t out[8])
{
    gpfq::PipeArgs pa;
    if (!out || !dense_layer_supported(N, m, C, alphabet, M, gpfq::options_snapshot(), &pa)) return 0;
    return gpfq::blk_instance_query(pa, out) ? 1 : 0;
}

size_t gpfq_dense_layer_workspace_bytes(int64_t N, int64_t m, int64_t C)
{
    return dense_layer_workspace_bytes(N, m, C, gpfq::options_snapshot());
}

// phase 0: the whole layer call; 1: the alphabet-independent half (status block, row norms, record pre-pass); 2: the alphabet-dependent half
static int dense_layer_impl(int phase, const float *X, const float *Xq, int64_t ld, const float *nrm32,
                            const float *W, int64_t ldc, int64_t c_lo, int64_t C,
                            const void *dev_alphabet, const double *unit_alphabet, int M,
                            int64_t N, int64_t m,
                            int8_t *qidx, float *Q, int out_layout, int64_t ldo, double *resid,
                            void *workspace, size_t workspace_bytes, void *stream, const char *what)
{
    if (N < 1 || m < 1 || C < 0 || c_lo < 0)
        return fail(GPFQ_ERR_INVALID_ARG, "bad size N=%lld m=%lld C=%lld c_lo=%lld", (long long)N, (long long)m, (long long)C, (long long)c_lo);
    HostAlphabet H;
    int rc = unit_alphabet_arg(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    if (C == 0) return GPFQ_OK;
    if (!X || !Xq) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (phase != 1 && (!W || !dev_alphabet)) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < m=%lld", (long long)ld, (long long)m);
    const gpfq::Options o = gpfq::options_snapshot();
    gpfq::PipeArgs pa{};
    pa.A = H.A; pa.N = N; pa.m = m; pa.C = C;
    pa.opt = o;
    if (phase != 1) {
        if (ldc < c_lo + C) return fail(GPFQ_ERR_INVALID_ARG, "kernel pitch ldc=%lld < c_lo + C=%lld", (long long)ldc, (long long)(c_lo + C));
        if (out_layout != GPFQ_LAYOUT_NEURON_MAJOR && out_layout != GPFQ_LAYOUT_KERAS) return fail(GPFQ_ERR_INVALID_ARG, "unknown output layout %d", out_layout);
        if (out_layout == GPFQ_LAYOUT_KERAS && ldo < c_lo + C) return fail(GPFQ_ERR_INVALID_ARG, "output pitch ldo=%lld < c_lo + C=%lld", (long long)ldo, (long long)(c_lo + C));
        if (out_layout == GPFQ_LAYOUT_KERAS && ldo != 1 && !gpfq::blk_keras_out_supported(pa))
            return fail(GPFQ_ERR_UNSUPPORTED, "the kernel of this shape (m=%lld, C=%lld) writes neuron-major outputs only (gpfq_dense_layer_keras_out_supported): "
                                              "ask for GPFQ_LAYOUT_NEURON_MAJOR and lay them out with gpfq_assemble_kernel_device", (long long)m, (long long)C);
    }
    gpfq::PipeArgs query;
    if (!dense_layer_supported(N, m, C, unit_alphabet, M, o, &query))
        return fail(GPFQ_ERR_UNSUPPORTED, "no block-pipelined kernel for N=%lld m=%lld C=%lld M=%d (gpfq_dense_layer_supported): use gpfq_quantize_neurons with a host alphabet",
                    (long long)N, (long long)m, (long long)C, M);
    if (!workspace || (uintptr_t)workspace % 16 != 0 || workspace_bytes < dense_layer_workspace_bytes(N, m, C, o))
        return fail(GPFQ_ERR_WORKSPACE, "%s needs %zu aligned workspace bytes", what, dense_layer_workspace_bytes(N, m, C, o));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    float *n32_out = nullptr;
    if (phase != 2) {
        // the call's counter block (exact fallbacks, cluster timeout, alphabet word) is zeroed with the row norms when they are formed here
        // (launch_blk: inside the record pre-pass, or by the row-norm kernel in front of it)
        if (!nrm32) {
            n32_out = reinterpret_cast<float *>(static_cast<char *>(workspace) + onchip_workspace_bytes(N, m, C, o));
        } else {
            e = hipMemsetAsync(workspace, 0, 64, s);
            if (e != hipSuccess) return hip_fail(e, what);
        }
    }
    pa.X = X; pa.Xq = Xq; pa.ld = ld; pa.nrm32 = nrm32; pa.nrm32_out = n32_out;
    pa.Wt = W ? W + c_lo : nullptr; pa.ldw = 1; pa.ldt = ldc;     // the Keras kernel itself: neuron j's weight of step t is W[t][c_lo + j]
    pa.resid = resid; pa.u_out = nullptr;
    if (out_layout == GPFQ_LAYOUT_KERAS) {
        pa.qidx = qidx ? qidx + c_lo : nullptr; pa.Qt = Q ? Q + c_lo : nullptr;
        pa.o_sj = 1; pa.o_st = ldo;
        if (ldo == 1) { pa.o_sj = N; pa.o_st = 1; }               // (a one-neuron layer: the two layouts coincide)
    } else {
        pa.qidx = qidx; pa.Qt = Q;
    }
    pa.dev_alpha = static_cast<const gpfq::DevAlphabet *>(dev_alphabet);
    pa.phase = phase;
    pa.workspace = static_cast<char *>(workspace) + onchip_stats_bytes(N);
    pa.fallback_count = static_cast<unsigned long long *>(workspace);
    if (phase == 2) {
        // the records in the workspace are the ones gpfq_dense_layer_prepare laid out: for the row of the kernel's table that THIS call resolves to?
        int prepared = -1, now = -1;
        if (!gpfq::blk_prepared_matches(pa, &prepared, &now))
            return fail(GPFQ_ERR_INVALID_ARG, "%s: the workspace was prepared for row %d of the block kernel's table, this call resolves to row %d "
                                              "(the options changed between gpfq_dense_layer_prepare and gpfq_dense_layer_run); nothing was computed", what, prepared, now);
    }
    e = gpfq::launch_blk(pa, s);
    if (e != hipSuccess) return hip_fail(e, what);
    if (phase == 1) gpfq::blk_note_prepared(pa);
    return (o.sync_errors && phase != 1) ? gpfq_call_status(workspace, stream) : GPFQ_OK;
}

int gpfq_quantize_dense_layer(const float *X, const float *Xq, int64_t ld, const float *nrm32,
                              const float *W, int64_t ldc, int64_t c_lo, int64_t C,
                              const void *dev_alphabet, const double *unit_alphabet, int M,
                              int64_t N, int64_t m,
                              int8_t *qidx, float *Q, int out_layout, int64_t ldo, double *resid,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    return dense_layer_impl(0, X, Xq, ld, nrm32, W, ldc, c_lo, C, dev_alphabet, unit_alphabet, M, N, m, qidx, Q, out_layout, ldo, resid,
                            workspace, workspace_bytes, stream, "gpfq_quantize_dense_layer");
}

int gpfq_dense_layer_prepare(const float *X, const float *Xq, int64_t ld, const float *nrm32, const double *unit_alphabet, int M,
                             int64_t N, int64_t m, int64_t C, void *workspace, size_t workspace_bytes, void *stream)
{
    return dense_layer_impl(1, X, Xq, ld, nrm32, nullptr, 0, 0, C, nullptr, unit_alphabet, M, N, m, nullptr, nullptr, GPFQ_LAYOUT_KERAS, 0, nullptr,
                            workspace, workspace_bytes, stream, "gpfq_dense_layer_prepare");
}

int gpfq_dense_layer_run(const float *X, const float *Xq, int64_t ld,
                         const float *W, int64_t ldc, int64_t c_lo, int64_t C,
                         const void *dev_alphabet, const double *unit_alphabet, int M,
                         int64_t N, int64_t m,
                         int8_t *qidx, float *Q, int out_layout, int64_t ldo, double *resid,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return dense_layer_impl(2, X, Xq, ld, nullptr, W, ldc, c_lo, C, dev_alphabet, unit_alphabet, M, N, m, qidx, Q, out_layout, ldo, resid,
                            workspace, workspace_bytes, stream, "gpfq_dense_layer_run");
}

int gpfq_assemble_kernel_device(const void *qidx, int bits, const void *dev_alphabet, int M, int64_t N, int64_t C,
                                float *Q, void *qidx_t, void *stream)
{
    if (N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size");
    if (bits != 2 && bits != 4 && bits != 8) return fail(GPFQ_ERR_INVALID_ARG, "bits must be 2, 4 or 8 (device-resident alphabets hold up to 64 members)");
    if (M < 1 || M > 64) return fail(GPFQ_ERR_UNSUPPORTED, "device-resident alphabets hold 1..64 members (got %d)", M);
    if (bits < 8 && M + 1 > (1 << bits)) return fail(GPFQ_ERR_INVALID_ARG, "%d-bit codes cannot hold an alphabet of %d", bits, M);
    if (N == 0 || C == 0) return GPFQ_OK;
    if (!qidx || !dev_alphabet) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (N > 2147483647LL * 32) return fail(GPFQ_ERR_UNSUPPORTED, "kernel too large to assemble in one call");
    gpfq::AlphabetArg A{};
    A.M = M;
    hipError_t e = gpfq::launch_assemble(static_cast<const int8_t *>(qidx), A, N, C, bits, Q, static_cast<int8_t *>(qidx_t),
                                         static_cast<hipStream_t>(stream), nullptr, static_cast<const gpfq::DevAlphabet *>(dev_alphabet));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_assemble_kernel_device");
}

size_t gpfq_gram_workspace_bytes(int64_t N, int64_t m, int64_t C)
{
    if (N < 0 || m < 0 || C < 0) return 0;
    return gpfq::gram_workspace_bytes(N, m, C);
}

int gpfq_quantize_neurons_gram(const float *X, const float *Xq, int64_t ld, float *nrm32, int compute_norms,
                               const float *Wt, int64_t ldw,
                               const double *alphabet, int M, int zero_idx,
                               int64_t N, int64_t m, int64_t C,
                               void *qidx, float *Qt, double *resid, int32_t *uncertified,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || m < 0 || C < 0)
        return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld m=%lld C=%lld", (long long)N, (long long)m, (long long)C);
    HostAlphabet H;
    int rc = make_alphabet(alphabet, M, zero_idx, &H);
    if (rc != GPFQ_OK) return rc;
    if (C == 0) return GPFQ_OK;
    if (N > GPFQ_GRAM_MAX_N) return fail(GPFQ_ERR_UNSUPPORTED, "Gram path needs N <= %d (got %lld)", GPFQ_GRAM_MAX_N, (long long)N);
    if (m >= (1LL << 30)) return fail(GPFQ_ERR_UNSUPPORTED, "Gram path needs m < 2^30 (error-bound derivation)");
    if (!uncertified) return fail(GPFQ_ERR_INVALID_ARG, "uncertified is NULL");
    if (N > 0 && (!Wt || !nrm32)) return fail(GPFQ_ERR_INVALID_ARG, "Wt/nrm32 is NULL");
    if (N > 0 && m > 0 && (!X || !Xq)) return fail(GPFQ_ERR_INVALID_ARG, "X/Xq is NULL");
    if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < m=%lld", (long long)ld, (long long)m);
    if (ldw < N) return fail(GPFQ_ERR_INVALID_ARG, "weight pitch ldw=%lld < N=%lld", (long long)ldw, (long long)N);
    const size_t need = gpfq::gram_workspace_bytes(N, m, C);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "Gram path needs %zu aligned workspace bytes", need);
    gpfq::GramArgs a;
    a.X = X; a.Xq = Xq; a.ld = ld; a.nrm32 = nrm32; a.Wt = Wt; a.ldw = ldw; a.A = H.A; a.big = H.big();
    a.N = N; a.m = m; a.C = C; a.qidx = static_cast<int8_t *>(qidx); a.Qt = Qt; a.resid = resid; a.uncertified = uncertified;
    a.workspace = workspace;
    a.nrm32_out = compute_norms ? nrm32 : nullptr;
    a.opt = gpfq::options_snapshot();
    a.slack = std::ldexp(1.0, a.opt.gram_slack_log2);
    // (noted like every other dense launch: a caller that asks gpfq_last_dense_kernel whether a deferred status exists -- the cluster
    //  form's -- must not see the name of an earlier call's kernel)
    gpfq::note_dense_kernel("gpfq_gram_* (Gram records + certified scalar recurrence)");
    hipError_t e = gpfq::launch_gram(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_neurons_gram");
}

int gpfq_msq_round(const float *W, int64_t n, const double *alphabet, int M, float *Q, void *qidx, void *stream)
{
    if (n < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative n");
    HostAlphabet H;
    int rc = make_alphabet(alphabet, M, -1, &H);
    if (rc != GPFQ_OK) return rc;
    if (n == 0) return GPFQ_OK;
    if (!W) return fail(GPFQ_ERR_INVALID_ARG, "W is NULL");
    hipError_t e = gpfq::launch_msq(W, n, H.A, Q, static_cast<int8_t *>(qidx), static_cast<hipStream_t>(stream), H.big());
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_msq_round");
}

int gpfq_index_bits(int M)
{
    if (M < 1 || M > GPFQ_MAX_ALPHABET) return 0;
    return M <= 3 ? 2 : (M <= 15 ? 4 : (M <= 64 ? 8 : 16));   // packed codes 0..M (0 = literal zero); plain int8 / int16 indices
}

int gpfq_pack_indices(const int8_t *qidx, int64_t N, int64_t C, int bits, uint8_t *packed, void *stream)
{
    if (N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size");
    if (bits != 2 && bits != 4) return fail(GPFQ_ERR_INVALID_ARG, "bits must be 2 or 4 (8-bit indices need no packing)");
    if (N == 0 || C == 0) return GPFQ_OK;
    if (!qidx || !packed) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    hipError_t e = gpfq::launch_pack(qidx, N, C, bits, packed, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_pack_indices");
}

int gpfq_assemble_kernel(const void *qidx, int bits, const double *alphabet, int M, int64_t N, int64_t C,
                         float *Q, void *qidx_t, void *stream)
{
    if (N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size");
    if (bits != 2 && bits != 4 && bits != 8 && bits != 16) return fail(GPFQ_ERR_INVALID_ARG, "bits must be 2, 4, 8 or 16");
    HostAlphabet H;
    int rc = make_alphabet(alphabet, M, -1, &H);
    if (rc != GPFQ_OK) return rc;
    if (bits < 8 && M + 1 > (1 << bits)) return fail(GPFQ_ERR_INVALID_ARG, "%d-bit codes cannot hold an alphabet of %d", bits, M);
    if ((bits == 16) != H.is_big)
        return fail(GPFQ_ERR_INVALID_ARG, "alphabets of %d members have %s indices (gpfq_index_bits)", M, H.is_big ? "int16" : "int8 or packed");
    if (N == 0 || C == 0) return GPFQ_OK;
    if (!qidx) return fail(GPFQ_ERR_INVALID_ARG, "qidx is NULL");
    if (N > 2147483647LL * 32) return fail(GPFQ_ERR_UNSUPPORTED, "kernel too large to assemble in one call");
    hipError_t e = gpfq::launch_assemble(static_cast<const int8_t *>(qidx), H.A, N, C, bits, Q, static_cast<int8_t *>(qidx_t),
                                         static_cast<hipStream_t>(stream), H.big());
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_assemble_kernel");
}

size_t gpfq_column_radii_workspace_bytes(int64_t R, int64_t C)
{
    (void)R; (void)C;
    return 0;                                  // a column never spans workgroups: nothing is handed between them
}

int gpfq_column_radii(const float *W, int64_t R, int64_t C, int64_t ld, double alphabet_scalar, const float *layer_median,
                      double *radii, float *W_scaled, int64_t ldo, int64_t c_lo, int64_t c_hi,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    (void)workspace; (void)workspace_bytes;
    if (R < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size R=%lld C=%lld", (long long)R, (long long)C);
    if (R > 2147483647LL) return fail(GPFQ_ERR_UNSUPPORTED, "columns of more than 2^31 - 1 rows");
    if (!(c_lo >= 0 && c_lo <= c_hi && c_hi <= C))
        return fail(GPFQ_ERR_INVALID_ARG, "scaled column range [%lld, %lld) outside [0, %lld]", (long long)c_lo, (long long)c_hi, (long long)C);
    if (C == 0) return GPFQ_OK;
    if (!radii) return fail(GPFQ_ERR_INVALID_ARG, "radii is NULL");
    if (R > 0 && !W) return fail(GPFQ_ERR_INVALID_ARG, "W is NULL");
    if (R > 0 && ld < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < C=%lld", (long long)ld, (long long)C);
    if (R > 0 && c_hi > c_lo) {
        if (!W_scaled) return fail(GPFQ_ERR_INVALID_ARG, "W_scaled is NULL with a column range to scale");
        if (ldo < C) return fail(GPFQ_ERR_INVALID_ARG, "W_scaled pitch ldo=%lld < C=%lld", (long long)ldo, (long long)C);
    }
    hipError_t e = gpfq::launch_column_radii(W, R, C, ld, alphabet_scalar, layer_median, radii, c_hi > c_lo ? W_scaled : nullptr, ldo,
                                             c_lo, c_hi, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_column_radii");
}

int gpfq_assemble_kernel_colrad(const void *qidx, int bits, int layout, const double *unit_alphabet, int M, const double *radii,
                                int64_t N, int64_t C, float *Q, void *qidx_t, void *stream)
{
    if (N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size");
    if (bits != 2 && bits != 4 && bits != 8 && bits != 16) return fail(GPFQ_ERR_INVALID_ARG, "bits must be 2, 4, 8 or 16");
    if (layout != GPFQ_LAYOUT_NEURON_MAJOR && layout != GPFQ_LAYOUT_KERAS) return fail(GPFQ_ERR_INVALID_ARG, "unknown index layout %d", layout);
    if (layout == GPFQ_LAYOUT_KERAS && bits < 8) return fail(GPFQ_ERR_INVALID_ARG, "packed indices are neuron-major rows (GPFQ_LAYOUT_NEURON_MAJOR)");
    HostAlphabet H;
    int rc = make_alphabet(unit_alphabet, M, -1, &H);
    if (rc != GPFQ_OK) return rc;
    if (bits < 8 && M + 1 > (1 << bits)) return fail(GPFQ_ERR_INVALID_ARG, "%d-bit codes cannot hold an alphabet of %d", bits, M);
    if ((bits == 16) != H.is_big)
        return fail(GPFQ_ERR_INVALID_ARG, "alphabets of %d members have %s indices (gpfq_index_bits)", M, H.is_big ? "int16" : "int8 or packed");
    if (N == 0 || C == 0) return GPFQ_OK;
    if (!qidx || !radii || !Q) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (N > 2147483647LL * 32) return fail(GPFQ_ERR_UNSUPPORTED, "kernel too large to assemble in one call");
    hipError_t e = gpfq::launch_assemble_colrad(qidx, bits, layout == GPFQ_LAYOUT_KERAS ? 1 : 0, H.A, H.big(), radii, N, C, Q,
                                                layout == GPFQ_LAYOUT_KERAS ? nullptr : qidx_t, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_assemble_kernel_colrad");
}

// ---- the packed low-bit form (gpfq_packed.hip) ----

int gpfq_packed_bits(int M, int zero_code) { return gpfq::packed_bits(M, zero_code); }

size_t gpfq_packed_row_bytes(int64_t R, int bits) { return gpfq::packed_row_bytes(R, bits); }

// The unit alphabet of a packed layer (1..64 members) and its (bits, zero_code) pair.
static int packed_alphabet(const double *unit_alphabet, int M, HostAlphabet *H)
{
    if (M > 64) return fail(GPFQ_ERR_UNSUPPORTED, "the packed form holds alphabets of at most 64 members, got M=%d", M);
    return make_alphabet(unit_alphabet, M, -1, H);
}

static int packed_width_ok(int bits, int zero_code, int M)
{
    if (bits != 2 && bits != 4 && bits != 8) return fail(GPFQ_ERR_INVALID_ARG, "bits must be 2, 4 or 8");
    if (zero_code != 0 && zero_code != 1) return fail(GPFQ_ERR_INVALID_ARG, "zero_code must be 0 or 1");
    if (M + zero_code > (1 << bits)) return fail(GPFQ_ERR_INVALID_ARG, "%d-bit codes cannot hold %d members%s", bits, M, zero_code ? " and the literal zero" : "");
    return GPFQ_OK;
}

int gpfq_encode_kernel(const float *Q, int64_t R, int64_t C, int64_t ld, const double *radii, const double *unit_alphabet, int M,
                       int8_t *idx, uint64_t *counters, void *stream)
{
    if (R < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size R=%lld C=%lld", (long long)R, (long long)C);
    HostAlphabet H;
    int rc = packed_alphabet(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    if (!counters) return fail(GPFQ_ERR_INVALID_ARG, "counters is NULL");
    if (R > 0 && C > 0) {
        if (!Q || !radii || !idx) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
        if (ld < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < C=%lld", (long long)ld, (long long)C);
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    hipError_t e = gpfq::launch_encode_kernel(Q, R, C, ld, radii, H.A, idx, reinterpret_cast<unsigned long long *>(counters),
                                              static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_encode_kernel");
}

int gpfq_pack_codes(const int8_t *idx, int64_t R, int64_t C, int bits, int zero_code, uint8_t *packed, void *stream)
{
    if (R < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size R=%lld C=%lld", (long long)R, (long long)C);
    int rc = packed_width_ok(bits, zero_code, 1);
    if (rc != GPFQ_OK) return rc;
    if (R == 0 || C == 0) return GPFQ_OK;
    if (!idx || !packed) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (reinterpret_cast<uintptr_t>(packed) % 4 != 0) return fail(GPFQ_ERR_INVALID_ARG, "packed must be 4-byte aligned (16 for the forward pass)");
    hipError_t e = gpfq::launch_pack_codes(idx, R, C, bits, zero_code, packed, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_pack_codes");
}

int gpfq_unpack_kernel(const uint8_t *packed, int bits, int zero_code, const double *radii, const double *unit_alphabet, int M,
                       int64_t R, int64_t C, float *Q, int64_t ldq, int8_t *idx, void *stream)
{
    if (R < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size R=%lld C=%lld", (long long)R, (long long)C);
    HostAlphabet H;
    int rc = packed_alphabet(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    rc = packed_width_ok(bits, zero_code, M);
    if (rc != GPFQ_OK) return rc;
    if (R == 0 || C == 0 || (!Q && !idx)) return GPFQ_OK;
    if (!packed || !radii) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (Q && ldq < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldq=%lld < C=%lld", (long long)ldq, (long long)C);
    hipError_t e = gpfq::launch_unpack_kernel(packed, bits, zero_code, radii, H.A, R, C, Q, ldq, idx, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_unpack_kernel");
}

// The forward entries: one set of checks for the arguments all three share (in: x, or xq for the int8 entry, with its row pitch), and
// the launcher of the kernel family named.  *nothing: an empty batch or layer, the call is done.
static int packed_forward_args(const void *in, const char *ld_name, int64_t ld, int64_t B, const uint8_t *packed,
                               int bits, int zero_code, const double *radii, int M, int64_t N, int64_t C, const float *y, int64_t ldy,
                               bool *nothing)
{
    *nothing = false;
    int rc = packed_width_ok(bits, zero_code, M);
    if (rc != GPFQ_OK) return rc;
    if (B == 0 || C == 0) {
        *nothing = true;
        return GPFQ_OK;
    }
    if (!y || !radii) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (ldy < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldy=%lld < C=%lld", (long long)ldy, (long long)C);
    if (N > 0) {
        if (!in || !packed) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
        if (ld < N) return fail(GPFQ_ERR_INVALID_ARG, "row pitch %s=%lld < N=%lld", ld_name, (long long)ld, (long long)N);
        if (reinterpret_cast<uintptr_t>(packed) % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "packed must be 16-byte aligned");
    }
    if (C > 2147483647LL * 8) return fail(GPFQ_ERR_UNSUPPORTED, "layer too wide for one launch");
    return GPFQ_OK;
}

typedef hipError_t (*PackedForwardLaunch)(const float *, int64_t, int64_t, const uint8_t *, int, int, const double *, const gpfq::AlphabetArg &,
                                          const float *, int64_t, int64_t, float *, int64_t, hipStream_t);

static int packed_forward_entry(const char *name, PackedForwardLaunch launch, const float *x, int64_t B, int64_t ldx, const uint8_t *packed,
                                int bits, int zero_code, const double *radii, const double *unit_alphabet, int M, const float *bias,
                                int64_t N, int64_t C, float *y, int64_t ldy, void *stream)
{
    if (B < 0 || N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size B=%lld N=%lld C=%lld", (long long)B, (long long)N, (long long)C);
    HostAlphabet H;
    int rc = packed_alphabet(unit_alphabet, M, &H);
    if (rc != GPFQ_OK) return rc;
    bool nothing;
    rc = packed_forward_args(x, "ldx", ldx, B, packed, bits, zero_code, radii, M, N, C, y, ldy, &nothing);
    if (rc != GPFQ_OK || nothing) return rc;
    hipError_t e = launch(x, B, ldx, packed, bits, zero_code, radii, H.A, bias, N, C, y, ldy, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, name);
}

int gpfq_packed_dense_forward(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                              const double *radii, const double *unit_alphabet, int M, const float *bias, int64_t N, int64_t C,
                              float *y, int64_t ldy, void *stream)
{
    return packed_forward_entry("gpfq_packed_dense_forward", gpfq::launch_packed_dense_forward, x, B, ldx, packed, bits, zero_code, radii,
                                unit_alphabet, M, bias, N, C, y, ldy, stream);
}

int gpfq_packed_dense_forward_tiled(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                    const double *radii, const double *unit_alphabet, int M, const float *bias, int64_t N, int64_t C,
                                    float *y, int64_t ldy, void *stream)
{
    return packed_forward_entry("gpfq_packed_dense_forward_tiled", gpfq::launch_packed_dense_forward_tiled, x, B, ldx, packed, bits,
                                zero_code, radii, unit_alphabet, M, bias, N, C, y, ldy, stream);
}

typedef hipError_t (*QuantizeRowsLaunch)(const float *, int64_t, int64_t, int64_t, int8_t *, int64_t, float *, hipStream_t);

// the checks, early returns and status codes of the quantizers of the activations (the row kernel, chunk = 0, and the split forms,
// whose chunks of a row must fit a grid dimension).  *nothing: an empty batch, the call is done.
static int quantize_rows_args(int64_t chunk, const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales,
                              bool *nothing)
{
    *nothing = false;
    if (B < 0 || N < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size B=%lld N=%lld", (long long)B, (long long)N);
    if (ldq % 16 != 0 || ldq < N) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldq=%lld must be a multiple of 16 and at least N=%lld", (long long)ldq, (long long)N);
    if (B == 0) {
        *nothing = true;
        return GPFQ_OK;
    }
    if (!scales) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (N > 0) {
        if (!x || !xq) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
        if (ldx < N) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldx=%lld < N=%lld", (long long)ldx, (long long)N);
        if (reinterpret_cast<uintptr_t>(xq) % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "xq must be 16-byte aligned");
    }
    if (B > 2147483647LL) return fail(GPFQ_ERR_UNSUPPORTED, "batch too long for one launch");
    if (chunk > 0 && N / chunk >= 2147483647LL) return fail(GPFQ_ERR_UNSUPPORTED, "row too long for one launch");
    return GPFQ_OK;
}

static int quantize_rows_entry(const char *name, QuantizeRowsLaunch launch, int64_t chunk, const float *x, int64_t B, int64_t ldx, int64_t N,
                               int8_t *xq, int64_t ldq, float *scales, void *stream)
{
    bool nothing;
    int rc = quantize_rows_args(chunk, x, B, ldx, N, xq, ldq, scales, &nothing);
    if (rc != GPFQ_OK || nothing) return rc;
    hipError_t e = launch(x, B, ldx, N, xq, ldq, scales, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, name);
}

int gpfq_quantize_rows_i8(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales, void *stream)
{
    return quantize_rows_entry("gpfq_quantize_rows_i8", gpfq::launch_quantize_rows_i8, 0, x, B, ldx, N, xq, ldq, scales, stream);
}

int gpfq_quantize_rows_i8_split(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales, void *stream)
{
    return quantize_rows_entry("gpfq_quantize_rows_i8_split", gpfq::launch_quantize_rows_i8_split, gpfq::quantize_split_chunk(), x, B, ldx, N,
                               xq, ldq, scales, stream);
}

int64_t gpfq_quantize_split_chunk(void) { return gpfq::quantize_split_chunk(); }

int gpfq_quantize_rows_i8_from_amax(const float *x, int64_t B, int64_t ldx, int64_t N, const uint32_t *amax_bits, int8_t *xq, int64_t ldq,
                                    float *scales, void *stream)
{
    bool nothing;
    int rc = quantize_rows_args(gpfq::quantize_split_chunk(), x, B, ldx, N, xq, ldq, scales, &nothing);
    if (rc != GPFQ_OK || nothing) return rc;
    if (!amax_bits) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    hipError_t e = gpfq::launch_quantize_rows_i8_from_amax(x, B, ldx, N, amax_bits, xq, ldq, scales, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_rows_i8_from_amax");
}

// both int8 Dense entries: the checks, early returns and status codes are the unfused entry's; fused adds relu and amax_bits
static int packed_dense_i8_entry(const char *name, bool fused, const int8_t *xq, int64_t B, int64_t ldq, const float *scales,
                                 const uint8_t *packed, int bits, int zero_code, const double *radii, int M, const float *bias, int64_t N,
                                 int64_t C, float *y, int64_t ldy, int relu, uint32_t *amax_bits, void *stream)
{
    if (relu != 0 && relu != 1) return fail(GPFQ_ERR_INVALID_ARG, "relu=%d: must be 0 or 1", relu);
    if (B < 0 || N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size B=%lld N=%lld C=%lld", (long long)B, (long long)N, (long long)C);
    if (M < 2 || M > 64) return fail(GPFQ_ERR_INVALID_ARG, "the int8 forward pass takes linspace(-1, 1, M) of 2..64 members, got M=%d", M);
    if (N > GPFQ_PACKED_I8_MAX_N)
        return fail(GPFQ_ERR_INVALID_ARG, "N=%lld > GPFQ_PACKED_I8_MAX_N=%d: the int32 sums could overflow", (long long)N, GPFQ_PACKED_I8_MAX_N);
    bool nothing;
    int rc = packed_forward_args(xq, "ldq", ldq, B, packed, bits, zero_code, radii, M, N, C, y, ldy, &nothing);
    if (rc != GPFQ_OK) return rc;
    if (B > 2147483647LL && amax_bits) return fail(GPFQ_ERR_UNSUPPORTED, "batch too long for one clear of amax_bits");
    if (nothing) {                                  // an empty layer still leaves its rows' cells cleared
        if (amax_bits && B > 0) {
            hipError_t e = gpfq::launch_amax_clear(amax_bits, B, static_cast<hipStream_t>(stream));
            if (e != hipSuccess) return hip_fail(e, name);
        }
        return GPFQ_OK;
    }
    if (!scales) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (ldq % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldq=%lld must be a multiple of 16", (long long)ldq);
    if (reinterpret_cast<uintptr_t>(xq) % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "xq must be 16-byte aligned");
    hipError_t e = fused ? gpfq::launch_packed_dense_forward_i8_fused(xq, B, ldq, scales, packed, bits, zero_code, radii, M, bias, N, C, y,
                                                                      ldy, relu, amax_bits, static_cast<hipStream_t>(stream))
                         : gpfq::launch_packed_dense_forward_i8(xq, B, ldq, scales, packed, bits, zero_code, radii, M, bias, N, C, y, ldy,
                                                                static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, name);
}

int gpfq_packed_dense_forward_i8(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                 int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                 int64_t ldy, void *stream)
{
    return packed_dense_i8_entry("gpfq_packed_dense_forward_i8", false, xq, B, ldq, scales, packed, bits, zero_code, radii, M, bias, N, C, y,
                                 ldy, 0, nullptr, stream);
}

int gpfq_packed_dense_forward_i8_fused(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                       int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                       int64_t ldy, int relu, uint32_t *amax_bits, void *stream)
{
    return packed_dense_i8_entry("gpfq_packed_dense_forward_i8_fused", true, xq, B, ldq, scales, packed, bits, zero_code, radii, M, bias, N,
                                 C, y, ldy, relu, amax_bits, stream);
}

// both int8 Conv2D entries, as packed_dense_i8_entry
static int packed_conv_i8_entry(const char *name, bool fused, const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits, void *stream)
{
    if (relu != 0 && relu != 1) return fail(GPFQ_ERR_INVALID_ARG, "relu=%d: must be 0 or 1", relu);
    if (n < 0 || F < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size n=%lld F=%lld", (long long)n, (long long)F);
    if (H <= 0 || W <= 0 || Cin <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad image shape H=%lld W=%lld Cin=%lld", (long long)H, (long long)W, (long long)Cin);
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || rh <= 0 || rw <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad kernel/stride/rate");
    if (M < 2 || M > 64) return fail(GPFQ_ERR_INVALID_ARG, "the int8 forward pass takes linspace(-1, 1, M) of 2..64 members, got M=%d", M);
    const int64_t K = (int64_t)kh * kw * Cin;       // (each factor checked below its own bound first: no overflow)
    if (kh > GPFQ_PACKED_I8_MAX_N || kw > GPFQ_PACKED_I8_MAX_N || Cin > GPFQ_PACKED_I8_MAX_N || (int64_t)kh * kw > GPFQ_PACKED_I8_MAX_N ||
        K > GPFQ_PACKED_I8_MAX_N)
        return fail(GPFQ_ERR_INVALID_ARG, "kh*kw*Cin=%d*%d*%lld > GPFQ_PACKED_I8_MAX_N=%d: the int32 sums could overflow", kh, kw,
                    (long long)Cin, GPFQ_PACKED_I8_MAX_N);
    int rc = packed_width_ok(bits, zero_code, M);
    if (rc != GPFQ_OK) return rc;
    if (bits != gpfq::packed_bits(M, zero_code))
        return fail(GPFQ_ERR_INVALID_ARG, "bits=%d, but %d members%s pack to %d bits (gpfq_packed_bits)", bits, M,
                    zero_code ? " and the literal zero" : "", gpfq::packed_bits(M, zero_code));
    if (ldq % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "image pitch ldq=%lld must be a multiple of 16", (long long)ldq);
    const int64_t oh = gpfq_patch_out_dim(H, kh, sh, rh, same_padding), ow = gpfq_patch_out_dim(W, kw, sw, rw, same_padding);
    if (n > 2147483647LL && amax_bits) return fail(GPFQ_ERR_UNSUPPORTED, "too many images for one clear of amax_bits");
    if (n == 0 || F == 0 || oh == 0 || ow == 0) {   // an empty layer still leaves its images' cells cleared
        if (amax_bits && n > 0) {
            hipError_t e = gpfq::launch_amax_clear(amax_bits, n, static_cast<hipStream_t>(stream));
            if (e != hipSuccess) return hip_fail(e, name);
        }
        return GPFQ_OK;
    }
    // what the kernel indexes with 32 bits: a place inside an image, a position, a tap's row and column
    const int64_t limit = 1LL << 24, keh = kh + (int64_t)(kh - 1) * (rh - 1), kew = kw + (int64_t)(kw - 1) * (rw - 1);
    if (H > limit || W > limit || sh > limit || sw > limit || keh > limit || kew > limit || H * W > 2147483647LL / Cin)
        return fail(GPFQ_ERR_UNSUPPORTED, "image, stride or dilated kernel too large for one launch");
    if (oh * ow > 0x7fff0000LL / n) return fail(GPFQ_ERR_UNSUPPORTED, "n*OH*OW output positions: too many for one launch");
    const int64_t ftiles = (F + 15) / 16, pblocks = (n * oh * ow + 63) / 64;
    if (ftiles > 2147483647LL / pblocks) return fail(GPFQ_ERR_UNSUPPORTED, "layer too wide for one launch");
    if (ldq < H * W * Cin) return fail(GPFQ_ERR_INVALID_ARG, "image pitch ldq=%lld < H*W*Cin=%lld", (long long)ldq, (long long)(H * W * Cin));
    if (!xq || !scales || !packed || !radii || !y) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (reinterpret_cast<uintptr_t>(xq) % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "xq must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(packed) % 16 != 0) return fail(GPFQ_ERR_INVALID_ARG, "packed must be 16-byte aligned");
    gpfq::ConvI8Shape S;
    S.H = (int)H; S.W = (int)W; S.Cin = (int)Cin; S.kh = kh; S.kw = kw; S.sh = sh; S.sw = sw; S.rh = rh; S.rw = rw;
    S.OH = (int)oh; S.OW = (int)ow;
    S.pad_top = S.pad_left = 0;
    if (same_padding) {
        // TF SAME: total = max((out-1)*stride + k_eff - in, 0), before = total / 2 (floor)
        int64_t th = (oh - 1) * sh + keh - H; if (th < 0) th = 0;
        int64_t tw = (ow - 1) * sw + kew - W; if (tw < 0) tw = 0;
        S.pad_top = (int)(th / 2);
        S.pad_left = (int)(tw / 2);
    }
    hipError_t e = fused ? gpfq::launch_packed_conv2d_forward_i8_fused(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y,
                                                                       relu, amax_bits, static_cast<hipStream_t>(stream))
                         : gpfq::launch_packed_conv2d_forward_i8(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y,
                                                                 static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, name);
}

int gpfq_packed_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                  int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                  const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                  const float *bias, int64_t F, float *y, void *stream)
{
    return packed_conv_i8_entry("gpfq_packed_conv2d_forward_i8", false, xq, n, ldq, scales, H, W, Cin, kh, kw, sh, sw, rh, rw, same_padding,
                                packed, bits, zero_code, radii, M, bias, F, y, 0, nullptr, stream);
}

int gpfq_packed_conv2d_forward_i8_fused(const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                        int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw,
                                        int same_padding, const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                        const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits, void *stream)
{
    return packed_conv_i8_entry("gpfq_packed_conv2d_forward_i8_fused", true, xq, n, ldq, scales, H, W, Cin, kh, kw, sh, sw, rh, rw,
                                same_padding, packed, bits, zero_code, radii, M, bias, F, y, relu, amax_bits, stream);
}

int gpfq_candidate_kernels(const float *W, int64_t R, int64_t C, int64_t ld, const double *base_radii, const float *layer_median,
                           const double *scalars, int K, double *radii, float *W_cand, int64_t ldo, int64_t c_lo, int64_t c_hi,
                           void *stream)
{
    if (R < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size R=%lld C=%lld", (long long)R, (long long)C);
    if (K < 1 || K > GPFQ_SEARCH_MAX_CANDIDATES)
        return fail(GPFQ_ERR_INVALID_ARG, "K=%d candidate scalars: must be 1..%d", K, GPFQ_SEARCH_MAX_CANDIDATES);
    if (!scalars) return fail(GPFQ_ERR_INVALID_ARG, "scalars is NULL");
    gpfq::SearchScalars S;
    std::memset(&S, 0, sizeof(S));
    S.K = K;
    for (int k = 0; k < K; ++k) {
        if (!(std::isfinite(scalars[k]) && scalars[k] > 0.0))
            return fail(GPFQ_ERR_INVALID_ARG, "candidate scalar %d is %g: every candidate must be a finite positive number", k, scalars[k]);
        S.s[k] = scalars[k];
    }
    if (!(c_lo >= 0 && c_lo <= c_hi && c_hi <= (int64_t)K * C))
        return fail(GPFQ_ERR_INVALID_ARG, "candidate column range [%lld, %lld) outside [0, %lld]", (long long)c_lo, (long long)c_hi,
                    (long long)((int64_t)K * C));
    if (C == 0) return GPFQ_OK;
    if (!radii) return fail(GPFQ_ERR_INVALID_ARG, "radii is NULL");
    if ((base_radii != nullptr) == (layer_median != nullptr))
        return fail(GPFQ_ERR_INVALID_ARG, "exactly one of base_radii (one per channel) and layer_median (one for the layer) must be given");
    const bool scale = R > 0 && c_hi > c_lo;
    if (scale) {
        if (!W) return fail(GPFQ_ERR_INVALID_ARG, "W is NULL");
        if (ld < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < C=%lld", (long long)ld, (long long)C);
        if (!W_cand) return fail(GPFQ_ERR_INVALID_ARG, "W_cand is NULL with a column range to write");
        if (ldo < (int64_t)K * C) return fail(GPFQ_ERR_INVALID_ARG, "W_cand pitch ldo=%lld < K * C=%lld", (long long)ldo, (long long)((int64_t)K * C));
    }
    hipError_t e = gpfq::launch_candidate_kernels(W, R, C, ld, base_radii, layer_median, S, radii, scale ? W_cand : nullptr, ldo, c_lo, c_hi,
                                                  static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_candidate_kernels");
}

size_t gpfq_select_candidates_workspace_bytes(int K, int64_t C)
{
    (void)K; (void)C;
    return GPFQ_SEARCH_MAX_CANDIDATES * sizeof(double);      // the K totals of per_layer, handed from the first launch to the second
}

int gpfq_select_candidates(const void *qidx, int bits, int64_t N, int64_t C, int K, int64_t T, const double *resid, const double *radii,
                           const double *unit_alphabet, int M, int per_layer, int32_t *best, double *scores, float *Q, void *qidx_sel,
                           double *radii_sel, double *resid_sel, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || C < 0 || T < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld C=%lld T=%lld", (long long)N, (long long)C, (long long)T);
    if (K < 1 || K > GPFQ_SEARCH_MAX_CANDIDATES)
        return fail(GPFQ_ERR_INVALID_ARG, "K=%d candidate scalars: must be 1..%d", K, GPFQ_SEARCH_MAX_CANDIDATES);
    if (bits != 8 && bits != 16) return fail(GPFQ_ERR_INVALID_ARG, "bits=%d: candidate indices are plain int8 (8) or int16 (16)", bits);
    HostAlphabet H;
    int rc = make_alphabet(unit_alphabet, M, -1, &H);
    if (rc != GPFQ_OK) return rc;
    if ((bits == 16) != H.is_big)
        return fail(GPFQ_ERR_INVALID_ARG, "alphabets of %d members have %s indices (gpfq_index_bits)", M, H.is_big ? "int16" : "int8");
    if (C == 0) return GPFQ_OK;
    if (!radii || !best || !scores) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer (radii, best and scores are required)");
    if (T > 0 && !resid) return fail(GPFQ_ERR_INVALID_ARG, "resid is NULL");
    if (N > 0 && (Q || qidx_sel) && !qidx) return fail(GPFQ_ERR_INVALID_ARG, "qidx is NULL with Q or qidx_sel to gather");
    if (per_layer && (!workspace || workspace_bytes < gpfq_select_candidates_workspace_bytes(K, C) || (uintptr_t)workspace % 8 != 0))
        return fail(GPFQ_ERR_WORKSPACE, "per-layer selection needs %zu aligned workspace bytes", gpfq_select_candidates_workspace_bytes(K, C));
    hipError_t e = gpfq::launch_select_candidates(qidx, bits, N, C, K, T, resid, radii, H.A, H.big(), per_layer ? 1 : 0, best, scores, Q,
                                                  qidx_sel, radii_sel, resid_sel, static_cast<double *>(workspace),
                                                  static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_select_candidates");
}

// ---- refinement sweeps after the walk (gpfq_refine.hip) ----

size_t gpfq_refine_workspace_bytes(int64_t N) { return gpfq::refine_workspace_bytes(N); }

int gpfq_refine_neurons_per_workgroup(int64_t m) { return gpfq::refine_neurons_per_workgroup(m); }

// What the three refinement entries refuse alike, each called at the place where the entry makes the check (the order of an entry's
// refusals is part of its contract: tests/golden/refine_refusals.json).
// The number of sweeps, then the unit alphabet, which goes into U, the kernels' argument (M and the members; the rest stays zero).
static int refine_sweeps_and_alphabet(int sweeps, const double *unit_alphabet, int M, gpfq::AlphabetBig *U)
{
    if (sweeps < 1) return fail(GPFQ_ERR_INVALID_ARG, "sweeps=%d must be >= 1", sweeps);
    HostAlphabet H;
    int rc = make_alphabet(unit_alphabet, M, -1, &H);
    if (rc != GPFQ_OK) return rc;
    U->M = M;
    for (int k = 0; k < M; ++k) U->a[k] = unit_alphabet[k];
    return GPFQ_OK;
}

// The pitches of the Keras-layout index and value arrays [N][C].
static int refine_keras_pitches(int64_t ldi, const float *Q, int64_t ldq, int64_t C)
{
    if (ldi < C) return fail(GPFQ_ERR_INVALID_ARG, "index pitch ldi=%lld < C=%lld", (long long)ldi, (long long)C);
    if (Q && ldq < C) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldq=%lld < C=%lld", (long long)ldq, (long long)C);
    return GPFQ_OK;
}

// Indices are int16 beyond 64 members.
static int refine_index_alignment(const gpfq::AlphabetBig &U, const void *qidx)
{
    if (U.M > 64 && (uintptr_t)qidx % 2 != 0) return fail(GPFQ_ERR_INVALID_ARG, "int16 indices must be 2-byte aligned");
    return GPFQ_OK;
}

int gpfq_refine_neurons(const float *X, const float *Xq, int64_t ld, const float *nrm32, const float *W, int64_t ldw,
                        const double *radii, const double *unit_alphabet, int M, int64_t N, int64_t m, int64_t C, int sweeps,
                        void *qidx, int64_t ldi, float *Q, int64_t ldq, double *resid_before, double *resid_after, int32_t *changed,
                        int32_t *sweeps_run, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || m < 0 || C < 0)
        return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld m=%lld C=%lld", (long long)N, (long long)m, (long long)C);
    gpfq::RefineArgs a{};
    int rc = refine_sweeps_and_alphabet(sweeps, unit_alphabet, M, &a.U);
    if (rc != GPFQ_OK) return rc;
    if (m > GPFQ_REFINE_MAX_M)
        return fail(GPFQ_ERR_UNSUPPORTED, "refinement needs m <= GPFQ_REFINE_MAX_M=%d (got %lld)", GPFQ_REFINE_MAX_M, (long long)m);
    if (N > 2147483647LL) return fail(GPFQ_ERR_UNSUPPORTED, "walks of more than 2^31 - 1 steps");
    if (C == 0) return GPFQ_OK;
    if (!radii) return fail(GPFQ_ERR_INVALID_ARG, "radii is NULL");
    if (N > 0) {
        if (!W || !nrm32 || !qidx) return fail(GPFQ_ERR_INVALID_ARG, "W/nrm32/qidx is NULL");
        if (m > 0 && (!X || !Xq)) return fail(GPFQ_ERR_INVALID_ARG, "X/Xq is NULL");
        if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < m=%lld", (long long)ld, (long long)m);
        if (ldw < C) return fail(GPFQ_ERR_INVALID_ARG, "weight pitch ldw=%lld < C=%lld", (long long)ldw, (long long)C);
        if ((rc = refine_keras_pitches(ldi, Q, ldq, C)) != GPFQ_OK || (rc = refine_index_alignment(a.U, qidx)) != GPFQ_OK) return rc;
        const size_t need = gpfq::refine_workspace_bytes(N);
        if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8 != 0)
            return fail(GPFQ_ERR_WORKSPACE, "refinement needs %zu aligned workspace bytes, got %zu", need, workspace ? workspace_bytes : (size_t)0);
    }
    a.X = X; a.Xq = Xq; a.ld = ld; a.nrm32 = nrm32; a.W = W; a.ldw = ldw; a.radii = radii;
    a.N = N; a.m = m; a.C = C; a.sweeps = sweeps; a.qidx = qidx; a.ldi = ldi; a.Q = Q; a.ldq = ldq;
    a.resid_before = resid_before; a.resid_after = resid_after; a.changed = changed; a.sweeps_run = sweeps_run;
    a.workspace = workspace;
    hipError_t e = gpfq::launch_refine(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_refine_neurons");
}

// ---- refinement sweeps on Gram matrices (gpfq_refine_gram.hip, DESIGN.md section 12 addendum) ----

int gpfq_refine_gram_neurons(const double *G, int64_t ldg, double *H, int64_t ldh, const float *nrm32, const double *radii,
                             const double *unit_alphabet, int M, int64_t N, int64_t C, int sweeps, void *qidx, int64_t ldi, float *Q,
                             int64_t ldq, int32_t *changed, int32_t *sweeps_run, double *gain, void *stream)
{
    if (N < 0 || C < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size N=%lld C=%lld", (long long)N, (long long)C);
    gpfq::RefineGramArgs a{};
    int rc = refine_sweeps_and_alphabet(sweeps, unit_alphabet, M, &a.U);
    if (rc != GPFQ_OK) return rc;
    if (N > GPFQ_REFINE_GRAM_MAX_N)
        return fail(GPFQ_ERR_UNSUPPORTED, "refinement on the Gram matrix needs N <= GPFQ_REFINE_GRAM_MAX_N=%d (got %lld)",
                    GPFQ_REFINE_GRAM_MAX_N, (long long)N);
    if (C > 2147483647LL) return fail(GPFQ_ERR_UNSUPPORTED, "more than 2^31 - 1 neurons in one call");
    if (C == 0) return GPFQ_OK;
    if (!radii) return fail(GPFQ_ERR_INVALID_ARG, "radii is NULL");
    if (N > 0) {
        if (!G || !H || !nrm32 || !qidx) return fail(GPFQ_ERR_INVALID_ARG, "G/H/nrm32/qidx is NULL");
        if (ldg < N) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldg=%lld < N=%lld", (long long)ldg, (long long)N);
        if (ldh < N) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ldh=%lld < N=%lld", (long long)ldh, (long long)N);
        if ((rc = refine_keras_pitches(ldi, Q, ldq, C)) != GPFQ_OK) return rc;
        if ((uintptr_t)G % 8 != 0 || (uintptr_t)H % 8 != 0) return fail(GPFQ_ERR_INVALID_ARG, "G and H must be 8-byte aligned");
        if ((rc = refine_index_alignment(a.U, qidx)) != GPFQ_OK) return rc;
    }
    a.G = G; a.ldg = ldg; a.H = H; a.ldh = ldh; a.nrm32 = nrm32; a.radii = radii;
    a.N = N; a.C = C; a.sweeps = sweeps; a.qidx = qidx; a.ldi = ldi; a.Q = Q; a.ldq = ldq;
    a.changed = changed; a.sweeps_run = sweeps_run; a.gain = gain;
    hipError_t e = gpfq::launch_refine_gram(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_refine_gram_neurons");
}

// ---- refinement sweeps per (input channel, filter) pair of a conv layer (gpfq_refine_pairs.hip) ----

int gpfq_refine_conv_pairs(const double *records, const double *records_swapped, int K, const float *Wt, const double *radii,
                           const double *unit_alphabet, int M, int64_t nch, int64_t F, int sweeps, void *qidx, float *Qt,
                           int32_t *changed, int32_t *sweeps_run, double *gain, void *stream)
{
    if (nch < 0 || F < 0) return fail(GPFQ_ERR_INVALID_ARG, "negative size nch=%lld F=%lld", (long long)nch, (long long)F);
    if (K < 1) return fail(GPFQ_ERR_INVALID_ARG, "K=%d must be >= 1", K);
    gpfq::RefinePairsArgs a{};
    int rc = refine_sweeps_and_alphabet(sweeps, unit_alphabet, M, &a.U);
    if (rc != GPFQ_OK) return rc;
    if (K > GPFQ_REFINE_PAIRS_MAX_K)
        return fail(GPFQ_ERR_UNSUPPORTED, "refinement per (channel, filter) pair needs kh*kw <= GPFQ_REFINE_PAIRS_MAX_K=%d (got %d)",
                    GPFQ_REFINE_PAIRS_MAX_K, K);
    if (nch == 0 || F == 0) return GPFQ_OK;
    if (nch > 2147483647LL / ((F + 63) / 64)) return fail(GPFQ_ERR_UNSUPPORTED, "more than 2^31 - 1 tiles of 64 pairs in one call");
    if (!records || !Wt || !radii || !qidx) return fail(GPFQ_ERR_INVALID_ARG, "records/Wt/radii/qidx is NULL");
    if ((uintptr_t)records % 8 != 0 || (uintptr_t)records_swapped % 8 != 0 || (uintptr_t)radii % 8 != 0)
        return fail(GPFQ_ERR_INVALID_ARG, "records and radii must be 8-byte aligned");
    if ((rc = refine_index_alignment(a.U, qidx)) != GPFQ_OK) return rc;
    a.records = records; a.records_swapped = records_swapped; a.K = K; a.Wt = Wt; a.radii = radii;
    a.nch = nch; a.F = F; a.sweeps = sweeps; a.qidx = qidx; a.Qt = Qt;
    a.changed = changed; a.sweeps_run = sweeps_run; a.gain = gain;
    hipError_t e = gpfq::launch_refine_pairs(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_refine_conv_pairs");
}

size_t gpfq_median_abs_workspace_bytes(void) { return gpfq::median_workspace_bytes() + 64; }
size_t gpfq_median_abs_workspace_bytes_for(int64_t n) { return n > 0 ? gpfq::median_workspace_bytes_fast(n) : gpfq::median_workspace_bytes() + 64; }

int gpfq_median_abs(const float *W, int64_t n, float *median_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n <= 0) return fail(GPFQ_ERR_INVALID_ARG, "median of %lld elements", (long long)n);
    if (!W || !median_out) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (!workspace || workspace_bytes < gpfq_median_abs_workspace_bytes() || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "median needs %zu aligned workspace bytes", gpfq_median_abs_workspace_bytes());
    hipError_t e = gpfq::launch_median_abs(W, n, median_out, workspace, static_cast<hipStream_t>(stream), workspace_bytes);
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_median_abs");
}

static int median_ws_ok(void *workspace, size_t workspace_bytes)
{
    if (!workspace || workspace_bytes < gpfq::median_workspace_bytes() || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "median needs %zu aligned workspace bytes", gpfq::median_workspace_bytes());
    return GPFQ_OK;
}

int gpfq_median_abs_begin(int64_t n_total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_total <= 0) return fail(GPFQ_ERR_INVALID_ARG, "median of %lld elements", (long long)n_total);
    int rc = median_ws_ok(workspace, workspace_bytes);
    if (rc != GPFQ_OK) return rc;
    hipError_t e = gpfq::launch_median_begin(n_total, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_median_abs_begin");
}

int gpfq_median_abs_count(const float *W_local, int64_t n_local, int64_t n_total, int pass, void *workspace, void *stream)
{
    if (n_local < 0 || n_total <= 0 || n_local > n_total || pass < 0 || pass > 2) return fail(GPFQ_ERR_INVALID_ARG, "bad slice/pass");
    if ((n_local > 0 && !W_local) || !workspace) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    hipError_t e = gpfq::launch_median_count(W_local, n_local, n_total, pass, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_median_abs_count");
}

int gpfq_median_abs_pick(int64_t n_total, int pass, void *workspace, void *stream)
{
    if (n_total <= 0 || pass < 0 || pass > 2 || !workspace) return fail(GPFQ_ERR_INVALID_ARG, "bad pass / NULL workspace");
    hipError_t e = gpfq::launch_median_pick(n_total, pass, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_median_abs_pick");
}

int gpfq_median_abs_end(int64_t n_total, void *workspace, float *median_out, void *stream)
{
    if (n_total <= 0 || !workspace || !median_out) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    hipError_t e = gpfq::launch_median_end(n_total, workspace, median_out, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_median_abs_end");
}

int64_t gpfq_patch_out_dim(int64_t in, int64_t k, int64_t stride, int64_t rate, int same_padding)
{
    if (in <= 0 || k <= 0 || stride <= 0 || rate <= 0) return 0;
    if (same_padding) return (in + stride - 1) / stride;                 // ceil(in / stride)
    const int64_t keff = k + (k - 1) * (rate - 1);
    const int64_t span = in - keff + 1;
    return span <= 0 ? 0 : (span + stride - 1) / stride;                 // ceil((in - k_eff + 1) / stride)
}

int gpfq_extract_patches(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c,
                         int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                         float *P, int64_t ldp, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || Cin <= 0 || c < 0 || c >= Cin)
        return fail(GPFQ_ERR_INVALID_ARG, "bad activation shape/channel");
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || rh <= 0 || rw <= 0)
        return fail(GPFQ_ERR_INVALID_ARG, "bad kernel/stride/rate");
    const int64_t oh = gpfq_patch_out_dim(H, kh, sh, rh, same_padding);
    const int64_t ow = gpfq_patch_out_dim(W, kw, sw, rw, same_padding);
    const int64_t cols = n * oh * ow;
    if (cols == 0) return GPFQ_OK;
    if (!act || !P) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (ldp < cols) return fail(GPFQ_ERR_INVALID_ARG, "patch pitch ldp=%lld < n*oh*ow=%lld", (long long)ldp, (long long)cols);
    int pad_top = 0, pad_left = 0;
    if (same_padding) {
        // TF SAME: total = max((out-1)*stride + k_eff - in, 0), before = total / 2 (floor)
        const int64_t keh = kh + (int64_t)(kh - 1) * (rh - 1), kew = kw + (int64_t)(kw - 1) * (rw - 1);
        int64_t th = (oh - 1) * sh + keh - H; if (th < 0) th = 0;
        int64_t tw = (ow - 1) * sw + kew - W; if (tw < 0) tw = 0;
        pad_top = (int)(th / 2);
        pad_left = (int)(tw / 2);
    }
    hipError_t e = gpfq::launch_extract_patches(act, n, H, W, Cin, c, kh, kw, sh, sw, rh, rw, pad_top, pad_left,
                                                oh, ow, P, ldp, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_extract_patches");
}

int64_t gpfq_patch_column(int64_t total, int64_t S, uint64_t seed, int64_t i) { return gpfq::patch_column(total, S, seed, i); }

int gpfq_gather_patch_columns(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int kh, int kw,
                              int sh, int sw, int rh, int rw, int same_padding, int64_t S, uint64_t seed,
                              float *Xw, float *Xq, int64_t ld, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || Cin <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad activation shape");
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || rh <= 0 || rw <= 0)
        return fail(GPFQ_ERR_INVALID_ARG, "bad kernel/stride/rate");
    const int64_t oh = gpfq_patch_out_dim(H, kh, sh, rh, same_padding);
    const int64_t ow = gpfq_patch_out_dim(W, kw, sw, rw, same_padding);
    const int64_t total = n * oh * ow, N = (int64_t)kh * kw * Cin;
    const bool sampled = S > 0 && S < total;
    const int64_t m = sampled ? S : total;
    if (ld < m) return fail(GPFQ_ERR_INVALID_ARG, "row pitch ld=%lld < %lld columns", (long long)ld, (long long)m);
    if (ld == 0) return GPFQ_OK;
    if (sampled && S > 0x7fffffffll) return fail(GPFQ_ERR_UNSUPPORTED, "S=%lld sampled columns: the column rule takes S < 2^31", (long long)S);
    const bool two = act_q != nullptr && act_q != act_w;
    if (!act_w || !Xw || (two && !Xq)) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (((N + 63) / 64) * ((ld + 63) / 64) > 0x7fffffffll)
        return fail(GPFQ_ERR_UNSUPPORTED, "%lld rows x %lld columns: more tiles than one launch takes", (long long)N, (long long)ld);
    int pad_top = 0, pad_left = 0;
    if (same_padding) {
        // TF SAME, as gpfq_extract_patches
        const int64_t keh = kh + (int64_t)(kh - 1) * (rh - 1), kew = kw + (int64_t)(kw - 1) * (rw - 1);
        int64_t th = (oh - 1) * sh + keh - H; if (th < 0) th = 0;
        int64_t tw = (ow - 1) * sw + kew - W; if (tw < 0) tw = 0;
        pad_top = (int)(th / 2);
        pad_left = (int)(tw / 2);
    }
    hipError_t e = gpfq::launch_gather_patch_columns(act_w, two ? act_q : nullptr, n, H, W, Cin, kh, kw, sh, sw, rh, rw, pad_top, pad_left,
                                                     oh, ow, S, seed, Xw, two ? Xq : nullptr, ld, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_gather_patch_columns");
}

int gpfq_channel_planes(const float *act, int64_t npos, int64_t Cin, int64_t c_lo, int64_t nch, float *planes, void *stream)
{
    if (npos < 0 || Cin <= 0 || c_lo < 0 || nch < 0 || c_lo + nch > Cin)
        return fail(GPFQ_ERR_INVALID_ARG, "bad channel range [%lld, %lld) of %lld", (long long)c_lo, (long long)(c_lo + nch), (long long)Cin);
    if (npos == 0 || nch == 0) return GPFQ_OK;
    if (!act || !planes) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    hipError_t e = gpfq::launch_channel_planes(act, npos, Cin, c_lo, nch, planes, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_channel_planes");
}

size_t gpfq_channel_sumsq_workspace_bytes(int64_t Cin) { return Cin > 0 ? gpfq::channel_sumsq_workspace_bytes(Cin) : 0; }

int gpfq_channel_sumsq(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, double *sumsq,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || Cin <= 0 || sh <= 0 || sw <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad shape or stride");
    if (!sumsq) return fail(GPFQ_ERR_INVALID_ARG, "NULL output");
    if (workspace_bytes < gpfq_channel_sumsq_workspace_bytes(Cin) || !workspace) return fail(GPFQ_ERR_WORKSPACE, "workspace too small");
    if (n > 0 && !act) return fail(GPFQ_ERR_INVALID_ARG, "NULL activations");
    hipError_t e = gpfq::launch_channel_sumsq(act, n, H, W, Cin, sh, sw, sumsq, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_channel_sumsq");
}

size_t gpfq_channel_dead_workspace_bytes(int64_t Cin) { return Cin > 0 ? gpfq::channel_dead_workspace_bytes(Cin) : 0; }

int gpfq_channel_dead(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, int64_t prefix_positions,
                      int32_t *dead, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || Cin <= 0 || sh <= 0 || sw <= 0 || prefix_positions < 0) return fail(GPFQ_ERR_INVALID_ARG, "bad shape, stride or prefix");
    if (!dead) return fail(GPFQ_ERR_INVALID_ARG, "NULL output");
    if (workspace_bytes < gpfq_channel_dead_workspace_bytes(Cin) || !workspace || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "workspace too small or misaligned");
    if (n > 0 && !act) return fail(GPFQ_ERR_INVALID_ARG, "NULL activations");
    hipError_t e = gpfq::launch_channel_dead(act, n, H, W, Cin, sh, sw, dead, workspace, prefix_positions, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_channel_dead");
}

size_t gpfq_conv1x1_workspace_bytes(int64_t Cin)
{
    return Cin > 0 ? gpfq_channel_dead_workspace_bytes(Cin) + (((size_t)Cin * sizeof(int32_t) + 255) & ~(size_t)255) : 0;
}

int gpfq_quantize_conv1x1(const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, const float *Wt, int64_t F,
                          const double *alphabet, int M, float *Q, void *qidx, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0 || Cin <= 0 || F < 0 || sh <= 0 || sw <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad shape or stride");
    HostAlphabet A;
    int rc = make_alphabet(alphabet, M, -1, &A);
    if (rc != GPFQ_OK) return rc;
    if (F == 0) return GPFQ_OK;
    if (!Wt || (!Q && !qidx)) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (n > 0 && !act_q) return fail(GPFQ_ERR_INVALID_ARG, "NULL activations");
    if (workspace_bytes < gpfq_conv1x1_workspace_bytes(Cin) || !workspace || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "workspace too small or misaligned");
    int zero_idx = -1;
    for (int k = 0; k < M; ++k)
        if (alphabet[k] == 0.0) zero_idx = k;
    int32_t *dead = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + gpfq_channel_dead_workspace_bytes(Cin));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = gpfq::launch_channel_dead(act_q, n, H, W, Cin, sh, sw, dead, workspace, 0, st);
    if (e == hipSuccess) e = gpfq::launch_msq(Wt, Cin * F, A.A, Q, static_cast<int8_t *>(qidx), st, A.big(), dead, F, zero_idx);
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_conv1x1");
}

static size_t al256c(size_t x) { return (x + 255) & ~(size_t)255; }

// Every conv channel-loop entry below asks gpfq::resolve_conv_form (gpfq_gram_conv.hip) which kernel runs and what it needs; none of
// them holds a rule about the forms.
size_t gpfq_conv_channels_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw,
                                          int rh, int rw, int same_padding, int64_t F, int want_resid)
{
    return gpfq::resolve_conv_form(n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, F, want_resid != 0, false, false, gpfq::options_snapshot()).workspace_bytes;
}

int gpfq_conv_form(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                   int want_resid, int nhwc, int same_act, int32_t out[8])
{
    if (!out) return 0;
    gpfq::conv_form_query(gpfq::resolve_conv_form(n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, 0, want_resid != 0, nhwc != 0, same_act != 0,
                                                  gpfq::options_snapshot()), out);
    return out[0] != gpfq::ConvForm::none ? 1 : 0;
}

// phase 0: the whole channel loop; 1: Gram records only (-> records, negflags); 2: decide from given records
static int conv_channels_impl(int phase, double *records, int32_t *negflags,
                              const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                              int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                              const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                              void *qidx_v, float *Qt, double *resid, int32_t *uncertified,
                              void *workspace, size_t workspace_bytes, void *stream, int64_t pix = 1)
{
    if (n < 0 || H <= 0 || W <= 0 || nch < 0 || F < 0) return fail(GPFQ_ERR_INVALID_ARG, "bad shape");
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || rh <= 0 || rw <= 0) return fail(GPFQ_ERR_INVALID_ARG, "bad kernel/stride/rate");
    HostAlphabet HA;
    if (phase != 1) {
        int rc = make_alphabet(alphabet, M, zero_idx, &HA);
        if (rc != GPFQ_OK) return rc;
    }
    const gpfq::AlphabetArg &A = HA.A;
    int8_t *qidx = static_cast<int8_t *>(qidx_v);          // int16 elements when HA.is_big
    const bool same_act = act_w == act_q;          // first layer: both networks see the raw data (:478-481)
    const gpfq::Options o = gpfq::options_snapshot();
    const gpfq::ConvForm f = gpfq::resolve_conv_form(n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, F, resid != nullptr, pix > 1, same_act, o);
    const int64_t cols = f.cols, K = f.K;
    if (phase && (!records || !negflags)) return fail(GPFQ_ERR_INVALID_ARG, "NULL records / negflags");
    if (nch == 0 || (F == 0 && phase != 1) || cols == 0) return GPFQ_OK;
    if (f.too_large) return fail(GPFQ_ERR_UNSUPPORTED, "needs kh*kw <= %d and n*oh*ow < 2^30", GPFQ_GRAM_MAX_N);
    if (!act_w || !act_q) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (phase != 1 && (!Wt || !qidx || !Qt || !uncertified)) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (phase && resid) return fail(GPFQ_ERR_UNSUPPORTED, "residual norms need the whole call");
    if (!workspace || workspace_bytes < f.workspace_bytes || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "conv channel loop needs %zu aligned workspace bytes", f.workspace_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (f.cls) {
    case gpfq::ConvForm::none:
        return fail(GPFQ_ERR_UNSUPPORTED, "NHWC activations: only the 7x7 / stride 2 / VALID shift-sum form reads them (gpfq_conv_channels_nhwc_supported)");
    case gpfq::ConvForm::image:
    case gpfq::ConvForm::shift: {
        // 3x3 / stride 1: Gram matrices of every channel straight from the planes, one batched decide launch
        gpfq::ImageGramArgs g;
        g.act_w = act_w; g.act_q = act_q; g.n = n; g.H = H; g.W = W; g.nch = nch; g.pad = same_padding ? 1 : 0;
        g.Wt = Wt; g.A = A; g.big = HA.big(); g.F = F; g.qidx = qidx; g.Qt = Qt; g.uncertified = uncertified;
        g.workspace = workspace;
        g.slack = std::ldexp(1.0, o.gram_slack_log2);
        g.opt = o;
        g.phase = phase; g.records = records; g.negflags = negflags;
        hipError_t e = gpfq::launch_gram_image(g, f, s);
        return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_conv_channels(fused)");
    }
    case gpfq::ConvForm::tile:
    case gpfq::ConvForm::mfma:
    case gpfq::ConvForm::s2: {
        // any other shape: the tile kernel gathers its patch rows from the planes (implicit im2col)
        gpfq::ConvGramArgs g;
        g.act_w = act_w; g.act_q = act_q; g.n = n; g.H = H; g.W = W; g.nch = nch;
        g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.rh = rh; g.rw = rw;
        g.Wt = Wt; g.A = A; g.big = HA.big(); g.F = F; g.qidx = qidx; g.Qt = Qt; g.uncertified = uncertified;
        g.workspace = workspace;
        g.slack = std::ldexp(1.0, o.gram_slack_log2);
        g.phase = phase; g.records = records; g.negflags = negflags; g.pix = pix;
        hipError_t e = gpfq::launch_gram_conv(g, f, s);
        return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_conv_channels(implicit)");
    }
    case gpfq::ConvForm::loop:
        break;
    }
    if (phase) return fail(GPFQ_ERR_UNSUPPORTED, "records in / out need a kernel shape the plane kernels take");
    const int64_t ldp = (cols + 3) & ~(int64_t)3;
    char *ws = static_cast<char *>(workspace);
    float *Pw = reinterpret_cast<float *>(ws);   ws += al256c((size_t)K * ldp * sizeof(float));
    float *Pq = reinterpret_cast<float *>(ws);   ws += al256c((size_t)K * ldp * sizeof(float));
    float *nrm = reinterpret_cast<float *>(ws);  ws += al256c((size_t)K * sizeof(float));
    const int64_t plane = n * H * W;
    for (int64_t c = 0; c < nch; ++c) {
        hipError_t e = gpfq::launch_extract_patches(act_w + c * plane, n, H, W, 1, 0, kh, kw, sh, sw, rh, rw, f.pad_top, f.pad_left,
                                                    f.oh, f.ow, Pw, ldp, s);
        if (e == hipSuccess && !same_act)
            e = gpfq::launch_extract_patches(act_q + c * plane, n, H, W, 1, 0, kh, kw, sh, sw, rh, rw, f.pad_top, f.pad_left,
                                             f.oh, f.ow, Pq, ldp, s);
        if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_conv_channels(patches)");
        gpfq::GramArgs a;
        a.X = Pw; a.Xq = same_act ? Pw : Pq; a.ld = ldp; a.nrm32 = nrm; a.nrm32_out = nrm;
        a.Wt = Wt + c * F * K; a.ldw = K; a.A = A; a.big = HA.big(); a.N = K; a.m = cols; a.C = F;
        a.qidx = HA.at(qidx, c * F * K); a.Qt = Qt + c * F * K; a.resid = resid ? resid + c * F : nullptr;
        a.uncertified = uncertified + c * F;
        a.workspace = ws;
        a.slack = std::ldexp(1.0, o.gram_slack_log2);
        a.opt = o;
        e = gpfq::launch_gram(a, s);
        if (e != hipSuccess) return hip_fail(e, "gpfq_quantize_conv_channels(gram)");
    }
    return GPFQ_OK;
}

int gpfq_conv3x3_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t nch)
{
    const gpfq::Options o = gpfq::options_snapshot();
    return o.conv_fused && o.conv_nhwc && gpfq::gram_image_nhwc_supported(n, H, W, nch, o) ? 1 : 0;
}

size_t gpfq_conv3x3_nhwc_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch, int64_t F)
{
    const gpfq::Options o = gpfq::options_snapshot();
    if (!gpfq::gram_image_nhwc_supported(n, H, W, nch, o) || F < 0) return 0;
    return gpfq::gram_image_nhwc_workspace_bytes(n, H, W, nch, F, o);
}

int gpfq_quantize_conv3x3_nhwc(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c_lo, int64_t nch,
                               const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                               void *qidx, float *Qt, int32_t *uncertified, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n <= 0 || H <= 0 || W <= 0 || Cin <= 0 || c_lo < 0 || nch < 0 || c_lo + nch > Cin || F < 0) return fail(GPFQ_ERR_INVALID_ARG, "bad shape");
    HostAlphabet HA;
    int rc = make_alphabet(alphabet, M, zero_idx, &HA);
    if (rc != GPFQ_OK) return rc;
    if (nch == 0 || F == 0) return GPFQ_OK;
    const gpfq::Options o = gpfq::options_snapshot();
    if (!gpfq::gram_image_nhwc_supported(n, H, W, nch, o)) return fail(GPFQ_ERR_UNSUPPORTED, "NHWC form needs images of 4 x 4 or more and 32+ channels");
    if (!act_w || !act_q || !Wt || !qidx || !Qt || !uncertified) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    const size_t need = gpfq::gram_image_nhwc_workspace_bytes(n, H, W, nch, F, o);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 16 != 0)
        return fail(GPFQ_ERR_WORKSPACE, "NHWC conv call needs %zu aligned workspace bytes", need);
    gpfq::ImageGramArgs g;
    g.act_w = act_w + c_lo; g.act_q = act_q + c_lo; g.nhwc_cin = Cin;
    g.n = n; g.H = H; g.W = W; g.nch = nch; g.pad = 1;
    g.Wt = Wt; g.A = HA.A; g.big = HA.big(); g.F = F; g.qidx = static_cast<int8_t *>(qidx); g.Qt = Qt; g.uncertified = uncertified;
    g.workspace = workspace;
    g.slack = std::ldexp(1.0, o.gram_slack_log2);
    g.opt = o;
    hipError_t e = gpfq::launch_gram_image_nhwc(g, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GPFQ_OK : hip_fail(e, "gpfq_quantize_conv3x3_nhwc");
}

int gpfq_conv_records_supported(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw,
                                int same_padding)
{
    const gpfq::ConvForm f = gpfq::resolve_conv_form(n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, 0, false, false, false, gpfq::options_snapshot());
    return f.cls != gpfq::ConvForm::none && f.cls != gpfq::ConvForm::loop ? 1 : 0;       // (the halves need a plane kernel)
}

int gpfq_quantize_conv_channels(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                                int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                void *qidx, float *Qt, double *resid, int32_t *uncertified,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    return conv_channels_impl(0, nullptr, nullptr, act_w, act_q, n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, Wt, alphabet, M,
                              zero_idx, F, qidx, Qt, resid, uncertified, workspace, workspace_bytes, stream);
}

int gpfq_conv_channels_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding)
{
    const gpfq::Options o = gpfq::options_snapshot();
    // (conv_planes_free = 0: the layer driver is to form channel planes first, whatever the kernels could read)
    return o.conv_planes_free && gpfq::resolve_conv_form(n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, 0, false, true, false, o).cls == gpfq::ConvForm::s2 ? 1 : 0;
}

int gpfq_quantize_conv_channels_nhwc(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c_lo,
                                     int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                     const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                     void *qidx, float *Qt, int32_t *uncertified, void *workspace, size_t workspace_bytes, void *stream)
{
    if (Cin <= 0 || c_lo < 0 || nch < 0 || c_lo + nch > Cin) return fail(GPFQ_ERR_INVALID_ARG, "bad channel range");
    if (!act_w || !act_q) return fail(GPFQ_ERR_INVALID_ARG, "NULL pointer");
    if (Cin == 1)                                                   // one channel: the tensor IS its plane
        return conv_channels_impl(0, nullptr, nullptr, act_w, act_q, n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, Wt, alphabet, M,
                                  zero_idx, F, qidx, Qt, nullptr, uncertified, workspace, workspace_bytes, stream);
    return conv_channels_impl(0, nullptr, nullptr, act_w + c_lo, act_q + c_lo, n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, Wt, alphabet,
                              M, zero_idx, F, qidx, Qt, nullptr, uncertified, workspace, workspace_bytes, stream, Cin);
}

int gpfq_conv_channel_records(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                              int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                              double *records, int32_t *negflags, void *workspace, size_t workspace_bytes, void *stream)
{
    return conv_channels_impl(1, records, negflags, act_w, act_q, n, H, W, nch, kh, kw, sh, sw, rh, rw, same_padding, nullptr, nullptr, 0,
                              -1, 0, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int gpfq_quantize_conv_channels_from_records(const double *records, const int32_t *negflags,
                                             const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                                             int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                             const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                             void *qidx, float *Qt, int32_t *uncertified,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    return conv_channels_impl(2, const_cast<double *>(records), const_cast<int32_t *>(negflags), act_w, act_q, n, H, W, nch, kh, kw, sh, sw,
                              rh, rw, same_padding, Wt, alphabet, M, zero_idx, F, qidx, Qt, nullptr, uncertified, workspace,
                              workspace_bytes, stream);
}

}  // extern "C"
