// Checks the FFT-based DCT kernels against the GEMM kernels (compiled from the product
// source) on the bench grid 640 x 480 x 32, forward and inverse along each axis: max
// |FFT - GEMM| / max |GEMM|, round trip |inv(fwd(x)) - x| / max |x|, and time per pass.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
//       -I../optical-flow-optimal-transport_amd/csrc dct_check.hip -o dct_check
#include "../optical-flow-optimal-transport_amd/csrc/foto_dct.hip"
#include <cstdio>
#include <vector>
namespace foto { void set_error(const char*, ...) {} }
using namespace foto;

int main() {
    const int Nt = 32, Ny = 480, Nx = 640;
    const size_t n = (size_t)Nt * Ny * Nx;
    std::vector<double> h(n), a(n), b(n);
    uint64_t st = 88172645463325252ull;
    for (size_t i = 0; i < n; ++i) {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        h[i] = (double)(st >> 11) / 9007199254740992.0 - 0.5;
    }
    double *x, *y, *z, *w;
    if (hipMalloc(&x, n * 8) || hipMalloc(&y, n * 8) || hipMalloc(&z, n * 8) || hipMalloc(&w, n * 8)) return 1;
    (void)hipMemcpy(x, h.data(), n * 8, hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    struct Ax { const char* name; int outer, len, inner; };
    const Ax axes[3] = {{"x", Nt * Ny, Nx, 1}, {"y", Nt, Ny, Nx}, {"t", 1, Nt, Ny * Nx}};
    int bad = 0;
    for (const Ax& ax : axes) {
        std::vector<double> C, CT, mu;
        dct_matrix(ax.len, C, CT, mu);
        double *dC, *dCT, *tab;
        const std::vector<double> t = fft_table(ax.len);
        if (hipMalloc(&dC, C.size() * 8) || hipMalloc(&dCT, CT.size() * 8) || hipMalloc(&tab, t.size() * 8)) return 1;
        (void)hipMemcpy(dC, C.data(), C.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(dCT, CT.data(), CT.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(tab, t.data(), t.size() * 8, hipMemcpyHostToDevice);
        for (int inv = 0; inv < 2; ++inv) {
            auto time = [&](auto f) {
                float best = 1e9;
                for (int r = 0; r < 10; ++r) {
                    (void)hipEventRecord(e0);
                    f();
                    (void)hipEventRecord(e1);
                    (void)hipEventSynchronize(e1);
                    float ms;
                    (void)hipEventElapsedTime(&ms, e0, e1);
                    if (ms < best) best = ms;
                }
                return best * 1e3;
            };
            const double tg = time([&] { (void)dct_axis(ax.outer, ax.len, ax.inner, inv ? dCT : dC, x, y, 0); });
            hipError_t ef = hipSuccess;
            const double tf = time([&] { ef = dct_fft_axis(ax.outer, ax.len, ax.inner, inv, tab, x, z, 0); });
            if (ef == hipErrorNotSupported) { printf("%s: no FFT path for n = %d (GEMM %7.1f us)\n", ax.name, ax.len, tg); break; }
            if (ef != hipSuccess) { printf("%s: fft path error %d\n", ax.name, (int)ef); return 3; }
            (void)hipMemcpy(a.data(), y, n * 8, hipMemcpyDeviceToHost);
            (void)hipMemcpy(b.data(), z, n * 8, hipMemcpyDeviceToHost);
            double mx = 0, md = 0;
            for (size_t i = 0; i < n; ++i) { mx = fmax(mx, fabs(a[i])); md = fmax(md, fabs(a[i] - b[i])); }
            // round trip through the FFT path
            (void)dct_fft_axis(ax.outer, ax.len, ax.inner, !inv, tab, z, w, 0);
            (void)hipMemcpy(b.data(), w, n * 8, hipMemcpyDeviceToHost);
            double mr = 0, mh = 0;
            for (size_t i = 0; i < n; ++i) { mh = fmax(mh, fabs(h[i])); mr = fmax(mr, fabs(b[i] - h[i])); }
            printf("%s %s: |fft-gemm|/max %.2e  round trip %.2e  gemm %7.1f us  fft %7.1f us\n", ax.name,
                   inv ? "inverse" : "forward", md / mx, mr / mh, tg, tf);
            if (md / mx > 1e-13 || mr / mh > 1e-13) bad = 1;
        }
        (void)hipFree(dC); (void)hipFree(dCT); (void)hipFree(tab);
    }
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    printf(bad ? "FAIL\n" : "OK\n");
    return bad;
}
