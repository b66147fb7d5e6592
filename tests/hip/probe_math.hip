// probe_math.hip -- calls the fp32 building blocks of vr_device_math.h and the transfer-function reads of
// vr_sampling.h on the GPU with chosen arguments (tests/test_gpu_device_math.py).  A stand-alone program: it is not
// part of libvrhip.so and adds nothing to the product's ABI.
//
//   probe_math REQUEST RESULT
//
// REQUEST, 32-bit little-endian words:  magic, n_tables, n_records,
//   then per table   tff_n, prefix_n, tff_n RGBA8 entries (one word each), prefix_n words,
//   then per record  op, count, table (index, or ~0 for none), count * n_in argument words (element-major).
// RESULT: magic, then per record count * n_out result words.  Floats travel as their bit patterns.  The operation
// ids and their (n_in, n_out) are those of oracle/vr_oracle.h (VRO_OP_*).
//
// One __global__ kernel per operation, one element per thread.  Every HIP status is checked: the first error is
// printed and ends the program with status 1 before anything else is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vr_device_math.h"
#include "vr_internal.h"
#include "vr_sampling.h"

namespace {

constexpr uint32_t kMagic = 0x4d525056u;
constexpr uint32_t kNoTable = 0xffffffffu;
constexpr int kThreads = 256;

#define PROBE_HIP(call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "probe_math: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                      \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

[[noreturn]] void die(const char *what)
{
    fprintf(stderr, "probe_math: %s\n", what);
    exit(1);
}

VR_DEV float F(uint32_t u) { return __uint_as_float(u); }
VR_DEV uint32_t U(float f) { return __float_as_uint(f); }

// a = this element's n_in argument words, o = its n_out result words
#define PROBE_KERNEL(name, NI, NO, ...)                                                              \
    __global__ __launch_bounds__(kThreads) void probe_##name(const uint32_t *in, uint32_t *out, uint32_t n, \
                                                             TfView tf)                              \
    {                                                                                                \
        const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;                            \
        if (i >= n) return;                                                                          \
        const uint32_t *a = in + (size_t)i * (NI);                                                   \
        uint32_t *o = out + (size_t)i * (NO);                                                        \
        (void)tf;                                                                                    \
        __VA_ARGS__                                                                                  \
    }

PROBE_KERNEL(logf, 1, 1, o[0] = U(vr_logf(F(a[0])));)
PROBE_KERNEL(powr, 2, 1, o[0] = U(vr_powr(F(a[0]), F(a[1])));)
PROBE_KERNEL(sincosf, 1, 2, float s, c; vr_sincosf(F(a[0]), &s, &c); o[0] = U(s); o[1] = U(c);)
PROBE_KERNEL(atan2f, 2, 1, o[0] = U(vr_atan2f(F(a[0]), F(a[1])));)
PROBE_KERNEL(acosf, 1, 1, o[0] = U(vr_acosf(F(a[0])));)
PROBE_KERNEL(normalize3, 3, 3, const f3 v = normalize3(mk3(F(a[0]), F(a[1]), F(a[2]))); o[0] = U(v.x); o[1] = U(v.y);
             o[2] = U(v.z);)
PROBE_KERNEL(len3, 3, 1, o[0] = U(len3(mk3(F(a[0]), F(a[1]), F(a[2]))));)
PROBE_KERNEL(dot3, 6, 1, o[0] = U(dot3(mk3(F(a[0]), F(a[1]), F(a[2])), mk3(F(a[3]), F(a[4]), F(a[5]))));)
PROBE_KERNEL(vmin, 2, 1, o[0] = U(vmin(F(a[0]), F(a[1])));)
PROBE_KERNEL(vmax, 2, 1, o[0] = U(vmax(F(a[0]), F(a[1])));)
PROBE_KERNEL(vclamp, 3, 1, o[0] = U(vclamp(F(a[0]), F(a[1]), F(a[2])));)
PROBE_KERNEL(lerpf, 3, 1, o[0] = U(lerpf(F(a[0]), F(a[1]), F(a[2])));)
PROBE_KERNEL(rng, 1, 1, o[0] = parallel_rng(a[0]);)
PROBE_KERNEL(rng3, 3, 1, o[0] = parallel_rng3(a[0], a[1], a[2]);)
PROBE_KERNEL(map_uint_float, 1, 1, o[0] = U(map_uint_float(a[0]));)
PROBE_KERNEL(tff_linear, 1, 4, const float4 r = tff_linear<false>(tf.tff, (int)tf.tff_n, F(a[0])); o[0] = U(r.x);
             o[1] = U(r.y); o[2] = U(r.z); o[3] = U(r.w);)
PROBE_KERNEL(tff_linear_raw, 1, 4, const float4 r = tff_linear<true>(tf.tff, (int)tf.tff_n, F(a[0])); o[0] = U(r.x);
             o[1] = U(r.y); o[2] = U(r.z); o[3] = U(r.w);)
PROBE_KERNEL(tff_alpha, 1, 1, o[0] = U(tff_linear_alpha<false>(tf.tff, (int)tf.tff_n, F(a[0])));)
PROBE_KERNEL(tff_alpha_raw, 1, 1, o[0] = U(tff_linear_alpha<true>(tf.tff, (int)tf.tff_n, F(a[0])));)
PROBE_KERNEL(prefix_nearest, 1, 1, o[0] = prefix_nearest(tf.prefix, tf.prefix_n, F(a[0]));)
PROBE_KERNEL(skip_test, 2, 1, o[0] = skip_test(tf, F(a[0]), F(a[1])) ? 1u : 0u;)

typedef void (*probe_fn)(const uint32_t *, uint32_t *, uint32_t, TfView);
struct Op {
    probe_fn fn;
    uint32_t n_in, n_out;
    int tables;   // 0 none, 1 transfer function, 2 transfer function and prefix sum
};
// in the order of VRO_OP_* (oracle/vr_oracle.h)
const Op kOps[] = {
    {probe_logf, 1, 1, 0},           {probe_powr, 2, 1, 0},          {probe_sincosf, 1, 2, 0},
    {probe_atan2f, 2, 1, 0},         {probe_acosf, 1, 1, 0},         {probe_normalize3, 3, 3, 0},
    {probe_len3, 3, 1, 0},           {probe_dot3, 6, 1, 0},          {probe_vmin, 2, 1, 0},
    {probe_vmax, 2, 1, 0},           {probe_vclamp, 3, 1, 0},        {probe_lerpf, 3, 1, 0},
    {probe_rng, 1, 1, 0},            {probe_rng3, 3, 1, 0},          {probe_map_uint_float, 1, 1, 0},
    {probe_tff_linear, 1, 4, 1},     {probe_tff_linear_raw, 1, 4, 1}, {probe_tff_alpha, 1, 1, 1},
    {probe_tff_alpha_raw, 1, 1, 1},  {probe_prefix_nearest, 1, 1, 2}, {probe_skip_test, 2, 1, 2},
};
constexpr uint32_t kNumOps = sizeof(kOps) / sizeof(kOps[0]);

struct Table {
    float4 *tff = nullptr;
    uint32_t tff_n = 0;
    uint32_t *prefix = nullptr;
    uint32_t prefix_n = 0;
};

std::vector<uint32_t> read_words(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open the request file");
    if (fseek(f, 0, SEEK_END)) die("cannot seek in the request file");
    const long bytes = ftell(f);
    if (bytes < 0 || bytes % 4 || fseek(f, 0, SEEK_SET)) die("bad request file size");
    std::vector<uint32_t> w((size_t)bytes / 4);
    if (!w.empty() && fread(w.data(), 4, w.size(), f) != w.size()) die("short read of the request file");
    fclose(f);
    return w;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: probe_math REQUEST RESULT");
    const std::vector<uint32_t> req = read_words(argv[1]);
    size_t pos = 0;
    auto need = [&](size_t n) {
        if (n > req.size() - pos) die("truncated request file");
    };
    need(3);
    if (req[0] != kMagic) die("bad magic");
    const uint32_t n_tables = req[1], n_records = req[2];
    pos = 3;

    std::vector<Table> tables(n_tables);
    for (Table &t : tables) {
        need(2);
        t.tff_n = req[pos];
        t.prefix_n = req[pos + 1];
        pos += 2;
        if (t.tff_n < 1 || t.tff_n > 4096 || t.prefix_n < 1 || t.prefix_n > 4096) die("bad table size");
        need((size_t)t.tff_n + t.prefix_n);
        // CL_UNORM_INT8 -> float: c / 255.0f, as vrhip_set_transfer_function converts the table
        const uint8_t *rgba8 = reinterpret_cast<const uint8_t *>(&req[pos]);
        std::vector<float4> table(t.tff_n);
        for (uint32_t i = 0; i < t.tff_n; ++i) {
            table[i].x = (float)rgba8[4 * i + 0] / 255.0f;
            table[i].y = (float)rgba8[4 * i + 1] / 255.0f;
            table[i].z = (float)rgba8[4 * i + 2] / 255.0f;
            table[i].w = (float)rgba8[4 * i + 3] / 255.0f;
        }
        pos += t.tff_n;
        PROBE_HIP(hipMalloc(&t.tff, t.tff_n * sizeof(float4)));
        PROBE_HIP(hipMemcpy(t.tff, table.data(), t.tff_n * sizeof(float4), hipMemcpyHostToDevice));
        PROBE_HIP(hipMalloc(&t.prefix, t.prefix_n * sizeof(uint32_t)));
        PROBE_HIP(hipMemcpy(t.prefix, &req[pos], t.prefix_n * sizeof(uint32_t), hipMemcpyHostToDevice));
        pos += t.prefix_n;
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out) die("cannot open the result file");
    if (fwrite(&kMagic, 4, 1, out) != 1) die("cannot write the result file");

    uint32_t *d_in = nullptr, *d_out = nullptr;
    size_t cap_in = 0, cap_out = 0;
    std::vector<uint32_t> res;
    for (uint32_t r = 0; r < n_records; ++r) {
        need(3);
        const uint32_t op = req[pos], count = req[pos + 1], ti = req[pos + 2];
        pos += 3;
        if (op >= kNumOps) die("unknown operation");
        if (count > (1u << 28)) die("record too large");
        const Op &o = kOps[op];
        if (o.tables ? ti >= n_tables : ti != kNoTable) die("bad table index");
        const size_t w_in = (size_t)count * o.n_in, w_out = (size_t)count * o.n_out;
        need(w_in);
        if (count == 0) continue;
        if (w_in > cap_in) {
            if (d_in) PROBE_HIP(hipFree(d_in));
            PROBE_HIP(hipMalloc(&d_in, w_in * 4));
            cap_in = w_in;
        }
        if (w_out > cap_out) {
            if (d_out) PROBE_HIP(hipFree(d_out));
            PROBE_HIP(hipMalloc(&d_out, w_out * 4));
            cap_out = w_out;
        }
        PROBE_HIP(hipMemcpy(d_in, &req[pos], w_in * 4, hipMemcpyHostToDevice));
        pos += w_in;
        TfView tf = {nullptr, 0, nullptr, 0};
        if (o.tables) {
            const Table &t = tables[ti];
            tf.tff = t.tff;
            tf.tff_n = t.tff_n;
            tf.prefix = t.prefix;
            tf.prefix_n = t.prefix_n;
        }
        const uint32_t blocks = (count + (uint32_t)kThreads - 1u) / (uint32_t)kThreads;
        hipLaunchKernelGGL(o.fn, dim3(blocks), dim3(kThreads), 0, 0, (const uint32_t *)d_in, d_out, count, tf);
        PROBE_HIP(hipGetLastError());
        PROBE_HIP(hipDeviceSynchronize());
        res.resize(w_out);
        PROBE_HIP(hipMemcpy(res.data(), d_out, w_out * 4, hipMemcpyDeviceToHost));
        if (fwrite(res.data(), 4, w_out, out) != w_out) die("cannot write the result file");
    }
    if (pos != req.size()) die("trailing words in the request file");
    if (fclose(out)) die("cannot close the result file");
    if (d_in) PROBE_HIP(hipFree(d_in));
    if (d_out) PROBE_HIP(hipFree(d_out));
    for (Table &t : tables) {
        PROBE_HIP(hipFree(t.tff));
        PROBE_HIP(hipFree(t.prefix));
    }
    return 0;
}
