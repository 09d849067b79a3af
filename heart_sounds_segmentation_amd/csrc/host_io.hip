// host_io.hip -- host code that launches no kernel: the RCCL all-gather shim, the recording packer and the CSV parser.
// C ABI: include/hssfsst.h.
#include "host_common.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <string>
#include <thread>

using namespace hssfsst::host;

extern "C" {

// ---- hssfsst_allgather: ncclAllGather through dlopen (no link-time dependency on RCCL)
namespace {
struct RcclApi {
    void* handle = nullptr;
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*error_string)(int) = nullptr;
    bool tried = false;
    std::string why;                                     // why RCCL is not available (dlerror() answers once: kept)
};
RcclApi& rccl_api()
{
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!api.tried) {
        api.tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            const char* e = dlerror();
            if (e && api.why.empty()) api.why = e;
        }
        if (api.handle) api.why = "symbol ncclAllGather missing";
        if (api.handle) {
            api.all_gather = reinterpret_cast<decltype(api.all_gather)>(dlsym(api.handle, "ncclAllGather"));
            api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(api.handle, "ncclGetErrorString"));
        }
    }
    return api;
}
}  // namespace

int hssfsst_allgather(const float* sendbuf, float* recvbuf, int64_t count, void* nccl_comm, void* stream, int timeout_ms)
{
    if (!sendbuf || !recvbuf || !nccl_comm || count < 0 || timeout_ms < 0) return fail(HSSFSST_EINVAL, "allgather: bad argument");
    if (count == 0) return 0;
    RcclApi& api = rccl_api();
    if (!api.all_gather) return fail(HSSFSST_EUNSUPPORTED, "allgather: RCCL (librccl.so.1: ncclAllGather) is not available: %s", api.why.empty() ? "dlopen failed" : api.why.c_str());
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kNcclFloat32 = 7;                      // ncclFloat (rccl.h)
    const int rc = api.all_gather(sendbuf, recvbuf, static_cast<size_t>(count), kNcclFloat32, nccl_comm, st);
    if (rc != 0) return fail(HSSFSST_EHIP, "allgather: ncclAllGather: %s", api.error_string ? api.error_string(rc) : "error");
    if (timeout_ms == 0) return 0;
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, st);
    const auto t0 = std::chrono::steady_clock::now();
    while (e == hipSuccess) {
        e = hipEventQuery(ev);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) break;
        e = hipSuccess;
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms) {
            (void)hipEventDestroy(ev);
            return fail(HSSFSST_EHIP, "allgather: the collective did not complete within %d ms (a rank is missing?); it is still enqueued on the stream and owns both buffers", timeout_ms);
        }
        std::this_thread::yield();
    }
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) return fail(HSSFSST_EHIP, "allgather: %s", hipGetErrorString(e));
    return 0;
}

int64_t hssfsst_pack_recordings(const float* const* ptrs, const int64_t* lens, int64_t count, int stride, int n,
                                float* stage, int64_t stage_cap, int64_t* starts, int64_t starts_cap, int threads)
{
    if (!ptrs || !lens || !stage || !starts || count < 0 || stride < 1 || n < 1)
        return fail(HSSFSST_EINVAL, "pack_recordings: bad argument");
    std::vector<int64_t> pos(static_cast<size_t>(count) + 1, 0);
    int64_t nf = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t T = lens[i];
        if (T < 0 || !ptrs[i]) return fail(HSSFSST_EINVAL, "pack_recordings: recording %lld is NULL or negative", static_cast<long long>(i));
        pos[i + 1] = pos[i] + T;
        // frame_signal: L = floor((T - n) / stride) frames, one fewer than fit; L <= 0 -> the single frame x[:n]
        int64_t L = (T - n >= 0) ? (T - n) / stride : -1;
        if (L <= 0) L = 1;
        if (nf + L > starts_cap) return fail(HSSFSST_EINVAL, "pack_recordings: more than %lld frames", static_cast<long long>(starts_cap));
        for (int64_t k = 0; k < L; ++k) starts[nf + k] = pos[i] + k * stride;
        nf += L;
    }
    const int64_t total = pos[count];
    if (total > stage_cap) return fail(HSSFSST_EINVAL, "pack_recordings: %lld samples exceed the staging capacity %lld",
                                       static_cast<long long>(total), static_cast<long long>(stage_cap));
    int nt = threads > 0 ? threads : static_cast<int>(total / (1 << 20)) + 1;     // one thread per 4 MB of float32
    if (nt > 8) nt = 8;
    if (nt > count) nt = static_cast<int>(count > 0 ? count : 1);
    auto work = [&](int t) {
        // thread t copies the recordings whose first sample falls into its share of the staging buffer
        const int64_t lo = total * t / nt, hi = total * (t + 1) / nt;
        for (int64_t i = 0; i < count; ++i)
            if (pos[i] >= lo && pos[i] < hi && lens[i] > 0) std::memcpy(stage + pos[i], ptrs[i], static_cast<size_t>(lens[i]) * sizeof(float));
    };
    if (nt <= 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    return nf;
}

int64_t hssfsst_parse_signal_csv(const char* text, int64_t len, float* signals, int64_t* labels, int64_t cap)
{
    if (!text || len < 0 || cap < 0 || (cap > 0 && (!signals || !labels))) return fail(HSSFSST_EINVAL, "parse_signal_csv: bad argument");
    const char* p = text;
    const char* end = text + len;
    while (p < end && *p != '\n') ++p;                  // skiprows=1
    if (p < end) ++p;
    int64_t rows = 0;
    while (p < end) {
        const char* eol = p;
        while (eol < end && *eol != '\n') ++eol;
        const char* q = p;
        while (q < eol && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
        if (q < eol) {                                  // non-empty line
            char* stop = nullptr;
            const double sig = std::strtod(q, &stop);
            if (stop == q || stop >= eol || *stop != ',')
                return fail(HSSFSST_EINVAL, "parse_signal_csv: malformed row %lld", static_cast<long long>(rows + 2));
            const char* l0 = stop + 1;
            const double lab = std::strtod(l0, &stop);
            if (stop == l0) return fail(HSSFSST_EINVAL, "parse_signal_csv: malformed label in row %lld", static_cast<long long>(rows + 2));
            if (rows < cap) { signals[rows] = static_cast<float>(sig); labels[rows] = static_cast<int64_t>(lab); }
            ++rows;
        }
        p = (eol < end) ? eol + 1 : end;
    }
    return rows;
}

}  // extern "C"
