// dispatch.hpp -- how a runtime option becomes a template argument of a kernel launch (host side only).
//
//   with_bool(flag, [&](auto B) { ... kernel<B()> ... });                 B is std::true_type / std::false_type
//   with_value<0, 1, 3, 2>(xmode, [&](auto V) { ... kernel<V()> ... });   the first listed value equal to xmode; the LAST one is the fallback
//   with_bools([&](auto A, auto B) { ... }, a, b);                        with_bool nested over a, b, ... (first flag outermost)
//
// Plain templates and generic lambdas: the calls inline to the chain of compares a hand-written if / else ladder is, and the body is
// instantiated once per listed value -- exactly the instantiations such a ladder spells out.
#pragma once

#include <type_traits>

namespace gmg {

template <class F>
inline void with_bool(bool flag, F &&f)
{
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

template <int V0, int... Vs, class F>
inline void with_value(int v, F &&f)
{
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else with_value<Vs...>(v, f);
}

template <class F>
inline void with_bools(F &&f)
{
  f();
}
template <class F, class... Bs>
inline void with_bools(F &&f, bool b0, Bs... bs)
{
  with_bool(b0, [&](auto B0) { with_bools([&](auto... rest) { f(B0, rest...); }, bs...); });
}

}   // namespace gmg
