// mcba_dispatch.h -- host only: a run-time value becomes a compile-time one.  with_*(value, f) calls the generic lambda f with a
// std::integral_constant that carries the value; nested calls around ONE hipLaunchKernelGGL replace a ladder of launches per level.
// Each helper lists the values it instantiates f for: nothing beyond them is compiled.
#pragma once
#include <type_traits>
#include "mcba_device.h"

namespace mcba {

template <int V> using int_c = std::integral_constant<int, V>;

// f(int_c<V>) for the first V of the list that equals v; the LAST value is the default
template <int V0, int... Vs, class F>
inline void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(int_c<V0>{});
  else if (v == V0) f(int_c<V0>{});
  else with_int<Vs...>(v, f);
}
template <class F>
inline void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{}); else f(std::false_type{});
}
template <class F>
inline void with_motion(int motion, F&& f) { with_int<MOTION_STATIC, MOTION_ROLLING, MOTION_HAND_EYE>(motion, f); }
template <class F>
inline void with_df(int DF, F&& f) { with_int<12, 6>(DF, f); }   // frame block: two poses (rolling shutter) or one

}  // namespace mcba
