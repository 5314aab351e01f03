// Probe: the device's logf / expf applied to the float32 values of a file, results to another -- the functions crit_partial_kernel and ew_kernel<EW_SIGMOID>
// (csrc/pointwise.hip) call, compiled with the library's flags, outside any kernel of the library.  tools/libm_ulp.py builds it, feeds it every argument
// tests/test_scalar_passes.py hands the two functions and compares with float64 log / exp; the bars of tests/test_scalar_passes_host.py carry what it measured.
// Likewise the four functions of csrc/intensity.hip: log2 / exp2 are the raw v_log_f32 / v_exp_f32 behind in_tail's t^g, log / cos the library calls of
// in_normal; tests/intensity_inputs.py carries what was measured on the arguments its cases produce.
// usage: libm_ulp_probe log|exp|log2|exp2|cos in.bin out.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

__global__ void apply(const float* x, float* y, size_t n, int op) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = x[i];
        y[i] = op == 0 ? logf(v) : op == 1 ? expf(v) : op == 2 ? __builtin_amdgcn_logf(v) : op == 3 ? __builtin_amdgcn_exp2f(v) : cosf(v);
    }
}

#define CK(e) do { hipError_t r = (e); if (r != hipSuccess) { fprintf(stderr, "hip: %s\n", hipGetErrorString(r)); return 2; } } while (0)

int main(int argc, char** argv) {
    if (argc != 4) return 1;
    const char* names[5] = {"log", "exp", "log2", "exp2", "cos"};
    int op = -1;
    for (int k = 0; k < 5; ++k)
        if (strcmp(argv[1], names[k]) == 0) op = k;
    if (op < 0) return 1;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / 4;
    fseek(f, 0, SEEK_SET);
    std::vector<float> h(n);
    if (fread(h.data(), 4, n, f) != n) return 1;
    fclose(f);
    float *dx, *dy;
    CK(hipMalloc(&dx, n * 4 + 4));
    CK(hipMalloc(&dy, n * 4 + 4));
    CK(hipMemcpy(dx, h.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(apply, dim3(1024), dim3(256), 0, 0, dx, dy, n, op);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), dy, n * 4, hipMemcpyDeviceToHost));
    f = fopen(argv[3], "wb");
    if (!f) return 1;
    fwrite(h.data(), 4, n, f);
    fclose(f);
    printf("%s of %zu values\n", argv[1], n);
    return 0;
}
