// Microbenchmark behind LAB_NOTEBOOK round 7: what one wave64 VALU instruction of the march's colour block costs a SIMD of gfx950 to issue.
// The colour block of march_accel_kernel is binary64 arithmetic (exact_expf), binary16 -> binary32 conversions and binary32 products;
// this prices them, and the instructions that can replace them, against v_fma_f32.
// Every wavefront runs `trips` times a unit of 256 instructions: 8 independent streams (no instruction waits for the one before it),
// unrolled 32 times, between two s_memtime reads.  Two launch shapes pin the occupancy through LDS: one 256-thread workgroup per compute
// unit (1 wavefront per SIMD: the instruction's own issue interval) and two 1024-thread workgroups (8 per SIMD: what the SIMD sustains).
// Prints cycles per wave64 instruction as the SIMD sees it: wavefront cycles / (instructions per wavefront * wavefronts per SIMD), and the
// same from the launch's wall time (which does not depend on both workgroups of a compute unit having run at the same time).
// Build + run on the GPU box: hipcc -O3 --offload-arch=gfx950 tools/micro/valu_issue_cost.hip -o /tmp/issue_cost && /tmp/issue_cost
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

enum Op { FMA_F32, MUL_F64, ADD_F64, FMA_F64, CVT_F64_F32, CVT_F32_F64, CVT_F32_F16, FMA_MIX_LO, FMA_MIX_HI, N_OPS };

template <int OP>
__device__ __forceinline__ void unit(float (&f)[8], double (&d)[8], float m, double md, uint32_t hw) {
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if constexpr (OP == FMA_F32) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(f[j]) : "v"(m));
            else if constexpr (OP == MUL_F64) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(d[j]) : "v"(md));
            else if constexpr (OP == ADD_F64) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[j]) : "v"(md));
            else if constexpr (OP == FMA_F64) asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(d[j]) : "v"(md));
            else if constexpr (OP == CVT_F64_F32) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[j]) : "v"(f[j]));
            else if constexpr (OP == CVT_F32_F64) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[j]) : "v"(d[j]));
            else if constexpr (OP == CVT_F32_F16) asm volatile("v_cvt_f32_f16 %0, %1" : "=v"(f[j]) : "v"(hw));
            else if constexpr (OP == FMA_MIX_LO) asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,0,0]" : "+v"(f[j]) : "v"(hw), "v"(m));
            else asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(f[j]) : "v"(hw), "v"(m));
        }
}

template <int OP>
__global__ __launch_bounds__(1024) void probe(int trips, float *sink, unsigned long long *clocks) {
    extern __shared__ char lds[];
    float f[8];
    double d[8];
    for (int j = 0; j < 8; ++j) {
        f[j] = 0.5f + 0.001f * (float)(threadIdx.x + j);
        d[j] = 0.5 + 0.001 * (double)(threadIdx.x + j);
    }
    const float m = 0.999f;
    const double md = 1.0;
    const uint32_t hw = 0x3c003800u + (threadIdx.x & 3u);  // binary16 1.0 (high half) and 0.5 (low half)
    if (threadIdx.x == 0) lds[0] = 0;
    __syncthreads();
    const unsigned long long c0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int u = 0; u < trips; ++u) unit<OP>(f, d, m, md, hw);
    const unsigned long long c1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    float s = 0.f;
    for (int j = 0; j < 8; ++j) s += f[j] + (float)d[j];
    if (s == 123.456f) sink[threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&clocks[0], c1 - c0);  // shader clock cycles (s_memtime) ...
        atomicAdd(&clocks[2], w1 - w0);  // ... and 100 MHz ticks (s_memrealtime) of the same interval
    }
}

template <int OP>
static void run(const char *name, int cus, int trips, float *sink, unsigned long long *clocks, hipEvent_t e0, hipEvent_t e1) {
    printf("%-28s", name);
    // {threads per workgroup, workgroups per CU, LDS bytes per workgroup}: 100 KB admits one workgroup per CU, 64 KB two
    const int shapes[2][3] = {{256, 1, 100 * 1024}, {1024, 2, 64 * 1024}};
    for (const auto &sh : shapes) {
        const int waves_per_simd = sh[0] / 256 * sh[1], blocks = cus * sh[1];
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(probe<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, sh[2]);
        hipLaunchKernelGGL(probe<OP>, dim3(blocks), dim3(sh[0]), sh[2], 0, trips / 10 + 1, sink, clocks);  // warm
        (void)hipMemset(clocks, 0, 32);
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(probe<OP>, dim3(blocks), dim3(sh[0]), sh[2], 0, trips, sink, clocks);
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        unsigned long long h[4];
        (void)hipMemcpy(h, clocks, 32, hipMemcpyDeviceToHost);
        const double waves = (double)blocks * (sh[0] / 64), instr = 256.0 * trips;
        // by the wavefronts' own clocks (right when every workgroup of the launch was resident at once), and by the launch's wall time
        // at the measured shader clock (right wherever the workgroups ran: instructions issued per SIMD over the launch's cycles)
        const double ghz = (double)h[0] / (double)h[2] * 0.1;
        printf("  %d/SIMD: %5.2f (by launch time %5.2f, %.2f GHz)", waves_per_simd, (double)h[0] / waves / instr / waves_per_simd,
               ms * 1e6 * ghz * (4.0 * cus) / (waves * instr), ghz);
    }
    printf("\n");
}

int main(int argc, char **argv) {
    const int trips = argc > 1 ? atoi(argv[1]) : 200;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) {
        fprintf(stderr, "no HIP device\n");
        return 1;
    }
    float *sink;
    unsigned long long *clocks;
    if (hipMalloc((void **)&sink, 4096) != hipSuccess || hipMalloc((void **)&clocks, 32) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    printf("cycles per wave64 instruction (s_memtime), %d compute units, %d trips of 256 instructions\n", cus, trips);
    run<FMA_F32>("v_fma_f32", cus, trips, sink, clocks, e0, e1);
    run<MUL_F64>("v_mul_f64", cus, trips, sink, clocks, e0, e1);
    run<ADD_F64>("v_add_f64", cus, trips, sink, clocks, e0, e1);
    run<FMA_F64>("v_fma_f64", cus, trips, sink, clocks, e0, e1);
    run<CVT_F64_F32>("v_cvt_f64_f32", cus, trips, sink, clocks, e0, e1);
    run<CVT_F32_F64>("v_cvt_f32_f64", cus, trips, sink, clocks, e0, e1);
    run<CVT_F32_F16>("v_cvt_f32_f16", cus, trips, sink, clocks, e0, e1);
    run<FMA_MIX_LO>("v_fma_mix_f32 (low half)", cus, trips, sink, clocks, e0, e1);
    run<FMA_MIX_HI>("v_fma_mix_f32 (high half)", cus, trips, sink, clocks, e0, e1);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
