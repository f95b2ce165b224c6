// +build cgo

/*
The bound-pod table's event path (include/bsched.h "the bound table patched in place"; INTEGRATION.md, preemption): a batch of bind /
delete events goes to the device as ONE call, bs_bound_apply_ex_flat with BS_BOUND_NODES, which moves the table and the node requests
together.  Nothing here is compiled in this repository's image (no Go toolchain); the call's behaviour is pinned by
tests/test_gpu_bound_apply_nodes.py through the same flat entry point.
*/
package core

/*
#include "bsched.h"
*/
import "C"

import "fmt"

// boundPodEvent is one pod that bound: the columns of a bound-table entry (bs_bound_delta's insert columns).
type boundPodEvent struct {
	node       uint32
	priority   int32
	startNs    int64
	group      int32
	req        []int64 // one value per lane of the context
	reqPresent uint32
	pdb        bool
}

// applyBoundEvents: one batch of bind / delete events as ONE call, bs_bound_apply_ex_flat with BS_BOUND_NODES — the ids in removed leave
// the bound table, the pods in bound arrive, and the node requests follow on the device (RemovePod per removed entry, AddPod per inserted
// one): the shim computes no request vector of its own.  A nominee of BS_PREEMPT_ASSUME that binds on its nominated node goes through
// with moveNodes == false (flags 0): its request is on the node already.  Returns the id of the first inserted entry; entry i gets
// first + i.
func (g *gpuCore) applyBoundEvents(removed []uint32, bound []boundPodEvent, lanes int, moveNodes bool) (uint32, error) {
	ni := len(bound)
	rem := make([]C.uint32_t, len(removed))
	for i, id := range removed {
		rem[i] = C.uint32_t(id)
	}
	node, pres := make([]C.uint32_t, ni), make([]C.uint32_t, ni)
	prio, group := make([]C.int32_t, ni), make([]C.int32_t, ni)
	start, req := make([]C.int64_t, ni), make([]C.int64_t, ni*lanes)
	pdb := make([]C.uint8_t, ni)
	for i, b := range bound {
		node[i], prio[i], start[i], group[i], pres[i] = C.uint32_t(b.node), C.int32_t(b.priority), C.int64_t(b.startNs), C.int32_t(b.group), C.uint32_t(b.reqPresent)
		for l := 0; l < lanes && l < len(b.req); l++ {
			req[l*ni+i] = C.int64_t(b.req[l]) // [L][n_insert]
		}
		if b.pdb {
			pdb[i] = 1
		}
	}
	var pRem, pNode, pPres *C.uint32_t
	var pPrio, pGroup *C.int32_t
	var pStart, pReq *C.int64_t
	var pPdb *C.uint8_t
	if len(rem) > 0 {
		pRem = &rem[0]
	}
	if ni > 0 {
		pNode, pPres, pPrio, pGroup, pStart, pPdb = &node[0], &pres[0], &prio[0], &group[0], &start[0], &pdb[0]
		if len(req) > 0 {
			pReq = &req[0]
		}
	}
	flags := C.uint32_t(0)
	if moveNodes {
		flags = C.BS_BOUND_NODES
	}
	var first C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_bound_apply_ex_flat(g.ctx, flags, C.uint32_t(len(rem)), pRem, C.uint32_t(ni), pNode, pPrio, pStart, pGroup, pReq, pPres, pPdb, &first); rc != C.BS_OK {
		return 0, fmt.Errorf("bs_bound_apply_ex_flat: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	return uint32(first), nil
}
