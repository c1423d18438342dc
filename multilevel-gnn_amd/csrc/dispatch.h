// Host-side value dispatch and pointer checks shared by every translation unit.  No HIP types: a plain C++17
// program can include this file (tests/test_dispatch_host.py does).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace mlgnn {

template <int V> using IC = std::integral_constant<int, V>;

// f(IC<V>{}) for the V of Vs... that equals v, then true.  A v that is not listed calls nothing and returns false:
// there is no default instantiation, the entry point answers MLGNN_E_SHAPE.
template <int... Vs, class F>
bool dispatch_int(int v, F&& f) {
  return ((v == Vs && (f(IC<Vs>{}), true)) || ...);
}

// A compile-time list of admitted values.  One list serves both sides of an entry point: the `_supported` predicate asks
// has(), the launcher dispatches over the same values, so the two cannot drift apart.
template <int... Vs>
struct IntList {
  static constexpr bool has(int64_t v) { return ((v == Vs) || ...); }
  template <class F>
  static bool dispatch(int v, F&& f) { return dispatch_int<Vs...>(v, std::forward<F>(f)); }
};

// every pointer a multiple of A bytes; a null pointer (an optional argument that is absent) counts as aligned
template <size_t A = 16, class... P>
bool aligned(const P*... p) {
  static_assert(A > 0 && (A & (A - 1)) == 0, "power of two");
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t{0}) & (A - 1)) == 0;
}

}  // namespace mlgnn
