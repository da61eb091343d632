// Per-axis DCT-II / DCT-III passes of the spectral solver (foto_dct.hip): what the plan calls.
#pragma once
#include <vector>

#include "foto_internal.h"

namespace foto {

// host tables: the orthonormal DCT-II matrix, its transpose and the eigenvalues mu; mu alone
void dct_matrix(int n, std::vector<double>& C, std::vector<double>& CT, std::vector<double>& mu);
void dct_eigen(int n, std::vector<double>& mu);
// FFT plans: whether n = 2 m1 m2 has one, and its per-axis table
bool fft_factors(int n, int* m1, int* m2);
std::vector<double> fft_table(int n);

// one axis of [outer][n][inner]: GEMM kernels (M: the n x n matrix) / FFT kernels (tab:
// fft_table; hipErrorNotSupported when n has no instantiation or tab is null -- a plan built
// with Tuning::dct_fft off uploads no tables)
hipError_t dct_axis(int outer, int n, int inner, const double* M, const double* in, double* out, hipStream_t s);
hipError_t dct_fft_axis(int outer, int n, int inner, bool inv, const double* tab, const double* in, double* out,
                        hipStream_t s);

}  // namespace foto
