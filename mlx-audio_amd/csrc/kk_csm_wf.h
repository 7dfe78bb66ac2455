// Weight formats of the CSM fragment packs (kk_csm_gemvm.h says what each holds): the template parameter FMT of gemvm_kernel / gemmp_kernel and
// KKCsmWeight::fmt (kk_kernels.h).  One definition for the library (kk_kernels.h includes it first) and for a stand-alone build of kk_csm_gemvm.h.
#pragma once
enum { KK_WF_BF16 = 0, KK_WF_Q8 = 1, KK_WF_Q4 = 2 };
