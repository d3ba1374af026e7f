// The step scheduler's top-k queue: std::priority_queue<NodeInfo> of JobInCtld::SchedulePendingSteps
// (src/CraneCtld/CtldPublicDefs.cpp:2056-2063) as libstdc++ builds it (bits/stl_heap.h: __push_heap / __adjust_heap / __pop_heap; see
// pq_emul.h for the annotated form), on an 8-byte entry.  Which of several nodes with the same task count leaves a full queue, and the
// order in which the nodes are handed their tasks, are artefacts of the heap layout; k_sched_steps (steps_kernels.hip) reproduces that
// layout move for move.  No HIP in here: tests/cpp/steps_host_test.cpp compiles this file with g++ and runs it against the real
// std::priority_queue at every size up to CNS_STEP_MAX_NODES + 1.
#pragma once
#include "res_dev.h"

namespace cns {

struct StepEnt { u32 ntasks; u32 pos; };   // NodeInfo {ntasks_on_node, craned_id} (:2056-2062)
// a < b  <=>  a.ntasks_on_node > b.ntasks_on_node (:2059-2061)
CNS_HD bool step_comp(const StepEnt& a, const StepEnt& b) { return a.ntasks > b.ntasks; }
// std::__push_heap / std::__adjust_heap of GCC's bits/stl_heap.h (see pq_emul.h for the annotated form)
CNS_HD void step_push_up(StepEnt* first, int hole, int top, StepEnt value) {
  int parent = (hole - 1) / 2;
  while (hole > top && step_comp(first[parent], value)) {
    first[hole] = first[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  first[hole] = value;
}
CNS_HD void step_pq_push(StepEnt* first, int len) { step_push_up(first, len - 1, 0, first[len - 1]); }
CNS_HD void step_pq_pop(StepEnt* first, int len) {  // len = size before the pop
  if (len <= 1) return;
  const StepEnt value = first[len - 1];
  first[len - 1] = first[0];
  const int n = len - 1;
  int hole = 0, child = 0;
  while (child < (n - 1) / 2) {
    child = 2 * (child + 1);
    if (step_comp(first[child], first[child - 1])) child--;
    first[hole] = first[child];
    hole = child;
  }
  if ((n & 1) == 0 && child == (n - 2) / 2) {
    child = 2 * (child + 1);
    first[hole] = first[child - 1];
    hole = child - 1;
  }
  step_push_up(first, hole, 0, value);
}

}  // namespace cns
