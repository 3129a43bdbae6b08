// Host side of the GEMM launchers: the runtime epilogue (and the 16-bit operand encoding) as template arguments.
#pragma once
#include <type_traits>
#include "common.h"

// epi_dispatch<EPI_BIAS, EPI_BIAS_GELU>(epi, "gemm_x: bad epilogue", f) calls f(std::integral_constant<int, E>{}) for the E of the list that
// equals epi and returns its result; an epilogue outside the list fails with `bad`.  Each kernel family lists exactly the epilogues it
// instantiates.
template <int... EPIS, typename F>
int epi_dispatch(int epi, const char* bad, F&& f) {
    int rc = 0;
    const bool hit = ((epi == EPIS && (rc = f(std::integral_constant<int, EPIS>{}), true)) || ...);
    return hit ? rc : s2v_fail(__FILE__, __LINE__, bad, -1);
}
// the same for the families with fp16 instantiations: f(epilogue, T16{}), T16 = f16_t for fp16 operands (GemmArgs::f16), bf16_t otherwise
template <int... EPIS, typename F>
int epi_dispatch16(int epi, bool f16, const char* bad, F&& f) {
    if (f16) return epi_dispatch<EPIS...>(epi, bad, [&](auto e) { return f(e, f16_t{}); });
    return epi_dispatch<EPIS...>(epi, bad, [&](auto e) { return f(e, bf16_t{}); });
}
