// auv_plan.h — the order of a shooting planner's candidates, shared by the scorer (k7_snapshot.hip: the argmax of auv_plan_score) and
// the refit (k15_plan.hip: the elite of auv_plan_refit).  Defined here alone.
#ifndef AUV_PLAN_H
#define AUV_PLAN_H
#include <hip/hip_runtime.h>

namespace {

// (score, index) a beats b: a valid score (not NaN) beats none; the larger score wins; the lower index wins a tie
#define PLAN_NONE 0x7fffffff
__device__ __forceinline__ bool plan_beats(const float sa, const int ia, const float sb, const int ib) {
  if (ia == PLAN_NONE) return false;
  if (ib == PLAN_NONE) return true;
  return sa > sb || (sa == sb && ia < ib);
}

// the TOTAL order plan_beats induces on the candidates of one group (ia != ib): a NaN score stands for "none", so it ranks below
// every number; NaNs order among themselves by index
__device__ __forceinline__ bool plan_ranks_before(const float sa, const int ia, const float sb, const int ib) {
  const bool na = sa != sa, nb = sb != sb;
  if (na && nb) return ia < ib;
  return plan_beats(sa, na ? PLAN_NONE : ia, sb, nb ? PLAN_NONE : ib);
}

}  // namespace
#endif /* AUV_PLAN_H */
