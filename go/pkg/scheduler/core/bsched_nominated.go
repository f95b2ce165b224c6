// +build cgo

/*
The resident nominated-pod table (include/bsched.h "the resident nominated-pod table"; INTEGRATION.md, preemption): pods that preempted
in an earlier cycle and have not bound yet.  The victim search of the three preemption calls counts them as upstream's
addNominatedPods does (rule N): for a preemptor of priority P, the rows on the node with priority >= P.  The shim keeps the row id
beside the pod's UID (preemptNominatedRead after a plan with BS_PREEMPT_NOMINATE) and removes a preemptor's OWN row before the pod is
searched for again: the table holds other pods' nominations.  Nothing here is compiled in this repository's image (no Go toolchain);
the calls' behaviour is pinned by tests/test_gpu_nominated.py through the same entry points, which take flat arguments only.
*/
package core

/*
#include "bsched.h"
*/
import "C"

import "fmt"

// nominatedRow is one nominee as loadNominated takes it and readNominated returns it.
type nominatedRow struct {
	id         uint32 // readNominated only: ids are 0 .. m-1 after a load
	node       uint32
	priority   int32
	req        []int64 // one value per lane of the context
	reqPresent uint32
}

// loadNominated: a snapshot (a restart; node-list surgery goes through nominatedFollowNodes and keeps the ids).  No rows: the empty
// table, which BS_PREEMPT_NOMINATE needs before its first call.
func (g *gpuCore) loadNominated(rows []nominatedRow, lanes int) error {
	m := len(rows)
	node, pres := make([]C.uint32_t, m), make([]C.uint32_t, m)
	prio, req := make([]C.int32_t, m), make([]C.int64_t, m*lanes)
	for i, r := range rows {
		node[i], prio[i], pres[i] = C.uint32_t(r.node), C.int32_t(r.priority), C.uint32_t(r.reqPresent)
		for l := 0; l < lanes && l < len(r.req); l++ {
			req[l*m+i] = C.int64_t(r.req[l]) // [L][m]
		}
	}
	var pNode, pPres *C.uint32_t
	var pPrio *C.int32_t
	var pReq *C.int64_t
	if m > 0 {
		pNode, pPrio, pReq, pPres = &node[0], &prio[0], &req[0], &pres[0]
	}
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_nominated_load(g.ctx, C.uint32_t(m), pNode, pPrio, pReq, pPres); rc != C.BS_OK {
		return g.pdbErr("bs_nominated_load", rc)
	}
	return nil
}

// applyNominated: the rows with the ids in removed leave (nominees that bound, were deleted, or are about to be searched for again);
// then one row per (podIndex[k], node[k], priority[k]) arrives, its request gathered on the device from the resident queue.  Returns
// the id of the first new row; row k gets first + k.
func (g *gpuCore) applyNominated(removed, podIndex, node []uint32, priority []int32) (uint32, error) {
	if len(podIndex) != len(node) || len(podIndex) != len(priority) {
		return 0, fmt.Errorf("applyNominated: %d pod indices, %d nodes, %d priorities", len(podIndex), len(node), len(priority))
	}
	_, pRem := u32s(removed)
	_, pPod := u32s(podIndex)
	_, pNode := u32s(node)
	_, pPrio := i32s(priority)
	var first C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_nominated_apply(g.ctx, C.uint32_t(len(removed)), pRem, C.uint32_t(len(podIndex)), pPod, pNode, pPrio, &first); rc != C.BS_OK {
		return 0, g.pdbErr("bs_nominated_apply", rc)
	}
	return uint32(first), nil
}

// readNominated: the table in table order (ascending id), for reconciliation.
func (g *gpuCore) readNominated(lanes int) ([]nominatedRow, error) {
	g.mu.Lock()
	defer g.mu.Unlock()
	var m C.uint32_t
	if rc := C.bs_nominated_count(g.ctx, &m); rc != C.BS_OK {
		return nil, g.pdbErr("bs_nominated_count", rc)
	}
	n := int(m)
	if n == 0 {
		return nil, nil
	}
	id, node, pres := make([]C.uint32_t, n), make([]C.uint32_t, n), make([]C.uint32_t, n)
	prio, req := make([]C.int32_t, n), make([]C.int64_t, n*lanes)
	if rc := C.bs_nominated_read(g.ctx, &id[0], &node[0], &prio[0], &req[0], &pres[0]); rc != C.BS_OK {
		return nil, g.pdbErr("bs_nominated_read", rc)
	}
	rows := make([]nominatedRow, n)
	for i := range rows {
		rows[i] = nominatedRow{id: uint32(id[i]), node: uint32(node[i]), priority: int32(prio[i]), reqPresent: uint32(pres[i]), req: make([]int64, lanes)}
		for l := 0; l < lanes; l++ {
			rows[i].req[l] = int64(req[l*n+i])
		}
	}
	return rows, nil
}

// droppedNominees: the rows of the nominated-pod table that left with their nodes, in ascending id.
type droppedNominees struct {
	id       []uint32 // the row's id: dead from now on
	node     []uint32 // the OLD index of the node it was nominated on
	priority []int32
}

// nominatedFollowNodes: bs_nominated_nodes_apply — the nominated-pod table follows node-list surgery on the device.  Called after the
// bs_nodes_apply call(s) it mirrors, with the kind and index fields of their deltas in order; bs_bound_nodes_apply and
// bs_wait_nodes_apply take the same two arrays, in any order among the three.  Rows on removed nodes leave and come back here: the shim
// clears those pods' NominatedNodeName and forgets their row ids; every other row keeps its id (the UID -> row id map stays valid) and
// names its node by the new index.  Every dropped row is taken back: the table holds at most BS_NOM_MAX rows.
func (g *gpuCore) nominatedFollowNodes(kind, index []uint32) (*droppedNominees, error) {
	if len(kind) != len(index) {
		return nil, fmt.Errorf("nominatedFollowNodes: %d kinds, %d indices", len(kind), len(index))
	}
	_, pKind := u32s(kind)
	_, pIndex := u32s(index)
	g.mu.Lock()
	defer g.mu.Unlock()
	var m, n C.uint32_t
	if rc := C.bs_nominated_count(g.ctx, &m); rc != C.BS_OK {
		return nil, g.pdbErr("bs_nominated_count", rc)
	}
	rows := int(m)
	oid, onode, oprio := make([]C.uint32_t, rows+1), make([]C.uint32_t, rows+1), make([]C.int32_t, rows+1)
	if rc := C.bs_nominated_nodes_apply(g.ctx, C.uint32_t(len(kind)), pKind, pIndex, C.uint32_t(rows), &oid[0], &onode[0], &oprio[0], &n); rc != C.BS_OK {
		return nil, g.pdbErr("bs_nominated_nodes_apply", rc)
	}
	k := int(n)
	d := &droppedNominees{id: make([]uint32, k), node: make([]uint32, k), priority: make([]int32, k)}
	for i := 0; i < k; i++ {
		d.id[i], d.node[i], d.priority[i] = uint32(oid[i]), uint32(onode[i]), int32(oprio[i])
	}
	return d, nil
}

// noNominatedRow is what preemptNominatedRead reports for a preemptor that got no node (or whose gang was voided).
const noNominatedRow = ^uint32(0)

// preemptNominatedRead: after a plan with BS_PREEMPT_NOMINATE, the row id of each preemptor in the caller's order.
func (g *gpuCore) preemptNominatedRead(count int) ([]uint32, error) {
	if count == 0 {
		return nil, nil
	}
	out := make([]C.uint32_t, count)
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_preempt_nominated_read(g.ctx, C.uint32_t(count), &out[0]); rc != C.BS_OK {
		return nil, g.pdbErr("bs_preempt_nominated_read", rc)
	}
	ids := make([]uint32, count)
	for i, x := range out {
		ids[i] = uint32(x)
	}
	return ids, nil
}

// consumedNominee is one row the nominated pass took off the table: the pod at queue index pod, whose row id was id, was assumed on node.
type consumedNominee struct {
	id, pod, node uint32
}

// seqPassNominated: seqPass with the nominated-pod table in the node choice (bs_seq_run_nominated, rule S of include/bsched.h): what
// upstream's podFitsOnNode does for every pod of the normal cycle.  priority[i] is the priority of queue pod i; ownRow[i] is the row id the
// shim keeps beside the pod's UID (preemptNominatedRead), noNominatedRow where the pod was never nominated; nil means nobody was.  A pod
// of priority P sees, on each node, the rows with priority >= P other than its own.  The rows of the pods the pass assumed — on whatever
// node, released or still waiting at Permit — have left the table when the call returns and come back in `consumed` (ascending id): the
// shim forgets those row ids (SchedulingQueue.DeleteNominatedPodIfExists); no bs_nominated_apply is needed for them.  The plugin's Filter
// stage is refused, as in the preemption calls.  Afterwards the context is where seqPass leaves it: bs_wait_park, bs_seq_expire and
// bs_bound_bind follow as usual.
func (g *gpuCore) seqPassNominated(priority []int32, ownRow []uint32) (*seqResult, []consumedNominee, error) {
	P := len(priority)
	if ownRow != nil && len(ownRow) != P {
		return nil, nil, fmt.Errorf("seqPassNominated: %d own rows for %d pods", len(ownRow), P)
	}
	cap := g.groups + 1
	r := &seqResult{pfCode: make([]C.uint8_t, P+1), podNode: make([]C.int32_t, P+1), releasedGroup: make([]C.uint32_t, cap),
		releasedPods: make([]C.uint32_t, cap), readyNs: make([]C.int64_t, cap), lastPermitted: make([]C.uint8_t, P+1)}
	firstNs := make([]C.int64_t, cap)
	var scalars [8]C.int64_t
	prio, own := make([]C.int32_t, P+1), make([]C.uint32_t, P+1)
	for i := range priority {
		prio[i] = C.int32_t(priority[i])
		own[i] = C.uint32_t(noNominatedRow)
		if ownRow != nil {
			own[i] = C.uint32_t(ownRow[i])
		}
	}
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_seq_run_nominated_flat(g.ctx, C.uint32_t(C.BS_STAGE_PREFILTER), C.uint32_t(P), &prio[0], &own[0], &r.pfCode[0], nil, nil,
		&r.podNode[0], C.uint32_t(cap), &r.releasedGroup[0], &r.releasedPods[0], &firstNs[0], &r.readyNs[0], &scalars[0],
		&r.lastPermitted[0]); rc != C.BS_OK {
		return nil, nil, g.pdbErr("bs_seq_run_nominated_flat", rc)
	}
	r.nReleased = int(scalars[0])
	var n C.uint32_t
	if rc := C.bs_seq_nominated_read(g.ctx, 0, nil, nil, nil, &n); rc != C.BS_OK {
		return nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	if n == 0 {
		return r, nil, nil
	}
	id, pod, node := make([]C.uint32_t, n), make([]C.uint32_t, n), make([]C.uint32_t, n)
	if rc := C.bs_seq_nominated_read(g.ctx, n, &id[0], &pod[0], &node[0], &n); rc != C.BS_OK {
		return nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	gone := make([]consumedNominee, n)
	for i := range gone {
		gone[i] = consumedNominee{uint32(id[i]), uint32(pod[i]), uint32(node[i])}
	}
	return r, gone, nil
}

// scoreWeights are the three weights of rule P (bs_seq_score): least requested, most requested, balanced allocation.
type scoreWeights struct {
	least, most, balanced uint32
}

// seqPassScoredNominated: seqPassNominated with the scored node choice (bs_seq_run_scored_nominated, rule SP of include/bsched.h): the
// pass a nominating cycle ends in.  The nominated-pod table decides which nodes are candidates (rule S: a pod of priority P sees the rows
// with priority >= P other than its own), rule P's total over the node's own requests decides among them — no row enters a score (D8) —,
// ties go to the lowest index.  priority, ownRow and `consumed` are seqPassNominated's.  total[i] is the chosen node's total and nFit[i]
// the number of candidates of queue pod i (bs_seq_score_read), 0 where the choice was not reached.
func (g *gpuCore) seqPassScoredNominated(w scoreWeights, priority []int32, ownRow []uint32) (r *seqResult, consumed []consumedNominee,
	total, nFit []uint32, err error) {
	P := len(priority)
	if ownRow != nil && len(ownRow) != P {
		return nil, nil, nil, nil, fmt.Errorf("seqPassScoredNominated: %d own rows for %d pods", len(ownRow), P)
	}
	cap := g.groups + 1
	r = &seqResult{pfCode: make([]C.uint8_t, P+1), podNode: make([]C.int32_t, P+1), releasedGroup: make([]C.uint32_t, cap),
		releasedPods: make([]C.uint32_t, cap), readyNs: make([]C.int64_t, cap), lastPermitted: make([]C.uint8_t, P+1)}
	firstNs := make([]C.int64_t, cap)
	var scalars [8]C.int64_t
	prio, own := make([]C.int32_t, P+1), make([]C.uint32_t, P+1)
	for i := range priority {
		prio[i] = C.int32_t(priority[i])
		own[i] = C.uint32_t(noNominatedRow)
		if ownRow != nil {
			own[i] = C.uint32_t(ownRow[i])
		}
	}
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_seq_run_scored_nominated_flat(g.ctx, C.uint32_t(C.BS_STAGE_PREFILTER), C.uint32_t(P), &prio[0], &own[0], C.uint32_t(w.least),
		C.uint32_t(w.most), C.uint32_t(w.balanced), &r.pfCode[0], nil, nil, &r.podNode[0], C.uint32_t(cap), &r.releasedGroup[0],
		&r.releasedPods[0], &firstNs[0], &r.readyNs[0], &scalars[0], &r.lastPermitted[0]); rc != C.BS_OK {
		return nil, nil, nil, nil, g.pdbErr("bs_seq_run_scored_nominated_flat", rc)
	}
	r.nReleased = int(scalars[0])
	ct, cf := make([]C.uint32_t, P+1), make([]C.uint32_t, P+1)
	if rc := C.bs_seq_score_read(g.ctx, C.uint32_t(P), &ct[0], &cf[0]); rc != C.BS_OK {
		return nil, nil, nil, nil, g.pdbErr("bs_seq_score_read", rc)
	}
	total, nFit = make([]uint32, P), make([]uint32, P)
	for i := 0; i < P; i++ {
		total[i], nFit[i] = uint32(ct[i]), uint32(cf[i])
	}
	var n C.uint32_t
	if rc := C.bs_seq_nominated_read(g.ctx, 0, nil, nil, nil, &n); rc != C.BS_OK {
		return nil, nil, nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	if n == 0 {
		return r, nil, total, nFit, nil
	}
	id, pod, node := make([]C.uint32_t, n), make([]C.uint32_t, n), make([]C.uint32_t, n)
	if rc := C.bs_seq_nominated_read(g.ctx, n, &id[0], &pod[0], &node[0], &n); rc != C.BS_OK {
		return nil, nil, nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	consumed = make([]consumedNominee, n)
	for i := range consumed {
		consumed[i] = consumedNominee{uint32(id[i]), uint32(pod[i]), uint32(node[i])}
	}
	return r, consumed, total, nFit, nil
}
