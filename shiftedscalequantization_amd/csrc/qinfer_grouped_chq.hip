// The per-channel (CHQ) instantiations of K25 / K26 (qinfer_grouped_kernels.h): this file alone is
// compiled without packed fp32 instructions (build.py, EXTRA_FLAGS), so the scalar kernels of
// qinfer_grouped.hip stay as they were built and measured.
#include "qinfer_grouped_kernels.h"

namespace ssq {

void qconv_dw_chq_launch(int64_t R, int64_t S, dim3 grid, hipStream_t stream, const int8_t* codes,
                         const int32_t* wc, const float* scale, const QDwGeo& g, const QEpiCh& e) {
  auto* kernel = qconv_dw_kernel<0, true, true>;
  if (R == S && R == 3) kernel = qconv_dw_kernel<3, true, true>;
  else if (R == S && R == 5) kernel = qconv_dw_kernel<5, true, true>;
  else if (R == S && R == 7) kernel = qconv_dw_kernel<7, true, true>;
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, codes, wc, scale, g, e);
}

void qconv_grouped_chq_launch(bool wide, dim3 grid, hipStream_t stream, const int8_t* codes,
                              const int8_t* wp, const int8_t* masks, const int32_t* cwz,
                              const int32_t* tt, const float* scale, const QGConvGeo& g,
                              const QEpiCh& e) {
  auto* kernel = wide ? qconv_grouped_kernel<true, true, true> : qconv_grouped_kernel<true, false, true>;
  hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, codes, wp, masks, cwz, tt, scale, g, e);
}

}  // namespace ssq
