// gsr_prims.h -- rocPRIM's two-call idiom (ask for the size of the temporary storage, reserve it, run), written once.  Apart from
// gsr_common.h so that the translation units without a scan or a sort do not parse rocPRIM.
#pragma once
#include <rocprim/rocprim.hpp>

#include "gsr_common.h"

namespace gsr {

// out[i] = in[0] + ... + in[i - 1] on stream `st`; `tmp` grows to what rocPRIM asks for
template <class Config, class T>
int32_t scan_exclusive(DevBuf& tmp, hipStream_t st, const T* in, T* out, size_t n) {
    size_t bytes = 0;
    GSR_HIP(rocprim::exclusive_scan<Config>(nullptr, bytes, in, out, (T)0, n, rocprim::plus<T>(), st));
    GSR_TRY(tmp.reserve(bytes));
    GSR_HIP(rocprim::exclusive_scan<Config>(tmp.p, bytes, in, out, (T)0, n, rocprim::plus<T>(), st));
    return GSR_OK;
}

// (kin, vin) sorted by bits [begin_bit, end_bit) of the key into (kout, vout).  The pointer types are the caller's own (a const
// input is another rocPRIM instantiation than a mutable one).
template <class Config, class KI, class KO, class VI, class VO>
int32_t sort_pairs_by_key(DevBuf& tmp, hipStream_t st, KI kin, KO kout, VI vin, VO vout, size_t n, unsigned begin_bit, unsigned end_bit) {
    size_t bytes = 0;
    GSR_HIP(rocprim::radix_sort_pairs<Config>(nullptr, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
    GSR_TRY(tmp.reserve(bytes));
    GSR_HIP(rocprim::radix_sort_pairs<Config>(tmp.p, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
    return GSR_OK;
}

}  // namespace gsr
