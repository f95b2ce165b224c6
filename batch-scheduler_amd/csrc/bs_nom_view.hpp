// bs_nom_view.hpp — the resident nominated-pod table (bs_nominated.hpp) as its READERS see it: the victim search of the preemption calls
// (rule N, bs_preempt.hpp) and the sequential pass of bs_seq_run_nominated (rule S, bs_seq.hpp).  One chain per node through the rows on
// it.  All null without a table or without rows.  The rows are static within a call.  The kernels get a POINTER to the view (it lives in the
// table's allocation; null = no rows): five fields in the kernel arguments cost every instantiation nine scalar registers for its whole
// life, and the pick and resolve kernels have none to spare.  Through the pointer the fields are scalar loads that live for the walk only.
#pragma once
#include <stdint.h>

namespace bs {

constexpr uint32_t kNmNone = 0xFFFFFFFFu;
struct NomView {
  const uint32_t* nhead;    // [n] first row on the node, kNmNone = none
  const uint32_t* nnext;    // [cap] next row on the same node
  const int32_t* nprio;     // [cap]
  const int64_t* nreq;      // [L][nstride] as AddPod counts the row
  uint32_t nstride;
};

}  // namespace bs
