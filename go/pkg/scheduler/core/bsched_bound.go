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

// Resident PodDisruptionBudgets (include/bsched.h "resident PodDisruptionBudgets"): the shim matches a pod's labels against the selectors
// once, when the pod binds, and hands the device the PDB indices; when a PDB's Status.PodDisruptionsAllowed changes, one
// bs_pdb_allowed_apply call rewrites the PDB bits on the device.  The shim keeps no label record per bound pod for this.

func u32s(v []uint32) ([]C.uint32_t, *C.uint32_t) {
	out := make([]C.uint32_t, len(v))
	for i, x := range v {
		out[i] = C.uint32_t(x)
	}
	if len(out) == 0 {
		return out, nil
	}
	return out, &out[0]
}

func i32s(v []int32) ([]C.int32_t, *C.int32_t) {
	out := make([]C.int32_t, len(v))
	for i, x := range v {
		out[i] = C.int32_t(x)
	}
	if len(out) == 0 {
		return out, nil
	}
	return out, &out[0]
}

func (g *gpuCore) pdbErr(what string, rc C.int) error {
	return fmt.Errorf("%s: %s (%s)", what, C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
}

// loadPDBs: after loadBound.  allowed[m] is PDB m's Status.PodDisruptionsAllowed; memberOff / member list, per bound-pod id, the PDBs
// that select the pod (len(memberOff) == ids + 1, from 0).
func (g *gpuCore) loadPDBs(allowed []int32, memberOff, member []uint32) error {
	b := 0
	if len(memberOff) > 0 {
		b = len(memberOff) - 1
	}
	_, pAllowed := i32s(allowed)
	_, pOff := u32s(memberOff)
	_, pMember := u32s(member)
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_pdb_load(g.ctx, C.uint32_t(len(allowed)), pAllowed, C.uint32_t(b), pOff, pMember); rc != C.BS_OK {
		return g.pdbErr("bs_pdb_load", rc)
	}
	return nil
}

// appendPDBMembers: after each applyBoundEvents that inserted pods: firstID is what it returned, memberOff (from 0) / member the PDBs
// of the inserted pods in the order they were inserted.
func (g *gpuCore) appendPDBMembers(firstID uint32, memberOff, member []uint32) error {
	n := 0
	if len(memberOff) > 0 {
		n = len(memberOff) - 1
	}
	_, pOff := u32s(memberOff)
	_, pMember := u32s(member)
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_pdb_members_append(g.ctx, C.uint32_t(firstID), C.uint32_t(n), pOff, pMember); rc != C.BS_OK {
		return g.pdbErr("bs_pdb_members_append", rc)
	}
	return nil
}

// applyPDBStatus: the PDBs whose Status.PodDisruptionsAllowed changed, each index once.
func (g *gpuCore) applyPDBStatus(index []uint32, allowed []int32) error {
	if len(index) != len(allowed) {
		return fmt.Errorf("applyPDBStatus: %d indices, %d values", len(index), len(allowed))
	}
	_, pIndex := u32s(index)
	_, pValue := i32s(allowed)
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_pdb_allowed_apply(g.ctx, C.uint32_t(len(index)), pIndex, pValue); rc != C.BS_OK {
		return g.pdbErr("bs_pdb_allowed_apply", rc)
	}
	return nil
}

// readPDBs: the resident budgets and the per-node violating counts (nodes = the node count), for reconciliation and tests.
func (g *gpuCore) readPDBs(nodes int) (allowed []int32, covered uint32, nodeViolating []uint32, err error) {
	var nPdb, cov C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_pdb_read(g.ctx, &nPdb, &cov, nil, nil); rc != C.BS_OK {
		return nil, 0, nil, g.pdbErr("bs_pdb_read", rc)
	}
	al := make([]C.int32_t, int(nPdb))
	nv := make([]C.uint32_t, nodes)
	var pAl *C.int32_t
	var pNv *C.uint32_t
	if len(al) > 0 {
		pAl = &al[0]
	}
	if len(nv) > 0 {
		pNv = &nv[0]
	}
	if rc := C.bs_pdb_read(g.ctx, nil, nil, pAl, pNv); rc != C.BS_OK {
		return nil, 0, nil, g.pdbErr("bs_pdb_read", rc)
	}
	allowed, nodeViolating = make([]int32, len(al)), make([]uint32, len(nv))
	for i, x := range al {
		allowed[i] = int32(x)
	}
	for i, x := range nv {
		nodeViolating[i] = uint32(x)
	}
	return allowed, uint32(cov), nodeViolating, nil
}

// gangPlan is what preemptCommitGang returns per preemptor (the caller's order) and per group.
type gangPlan struct {
	node        []int32  // nominated node, -1: none (also for a slot whose run was voided)
	nVictims    []uint32 // the true victim count; victims holds min(nVictims, victimCap) ids per row
	victims     []uint32 // [count][victimCap] bound-pod ids, zero beyond the row's count
	slotVoided  []uint8  // 1: the preemptor had a node and lost it to its gang's quorum
	groupPlaced []uint32 // per group: members of its run that got a node, before the decision
}

// preemptCommitGang: bs_preempt_commit_gang_flat, then bs_preempt_gang_read.  podIndex / priority list the preemptors with every gang's
// members next to each other (equal priorities: one run of slots per gang); gangNeed[g] is how many members of group g must get a node
// in this call (MinMember - Scheduled - the members already waiting at Permit; 0: no requirement) — a gang that misses it evicts nobody
// and holds no room.  flags: 0 (the plan), BS_PREEMPT_APPLY, BS_PREEMPT_APPLY | BS_PREEMPT_ASSUME, as for bs_preempt_commit.
func (g *gpuCore) preemptCommitGang(podIndex []uint32, priority []int32, groupProtected []uint8, gangNeed []uint32, flags uint32, victimCap uint32) (*gangPlan, error) {
	count := len(podIndex)
	if len(priority) != count || len(gangNeed) != len(groupProtected) {
		return nil, fmt.Errorf("preemptCommitGang: %d pod indices, %d priorities; %d needs, %d groups", count, len(priority), len(gangNeed), len(groupProtected))
	}
	_, pPod := u32s(podIndex)
	_, pPrio := i32s(priority)
	_, pNeed := u32s(gangNeed)
	prot := make([]C.uint8_t, len(groupProtected))
	var pProt *C.uint8_t
	for i, v := range groupProtected {
		prot[i] = C.uint8_t(v)
	}
	if len(prot) > 0 {
		pProt = &prot[0]
	}
	node := make([]C.int32_t, count+1)
	nv := make([]C.uint32_t, count+1)
	vic := make([]C.uint32_t, count*int(victimCap)+1)
	voided := make([]C.uint8_t, count+1)
	placed := make([]C.uint32_t, len(gangNeed)+1)
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_preempt_commit_gang_flat(g.ctx, C.BS_STAGE_PREFILTER, C.uint32_t(count), pPod, pPrio, pProt, pNeed, C.uint32_t(flags), C.uint32_t(victimCap),
		&node[0], nil, &nv[0], &vic[0], nil, nil, nil); rc != C.BS_OK {
		return nil, fmt.Errorf("bs_preempt_commit_gang_flat: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	if rc := C.bs_preempt_gang_read(g.ctx, C.uint32_t(count), &voided[0], C.uint32_t(len(gangNeed)), &placed[0]); rc != C.BS_OK {
		return nil, fmt.Errorf("bs_preempt_gang_read: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	p := &gangPlan{node: make([]int32, count), nVictims: make([]uint32, count), victims: make([]uint32, count*int(victimCap)),
		slotVoided: make([]uint8, count), groupPlaced: make([]uint32, len(gangNeed))}
	for i := 0; i < count; i++ {
		p.node[i], p.nVictims[i], p.slotVoided[i] = int32(node[i]), uint32(nv[i]), uint8(voided[i])
	}
	for i := range p.victims {
		p.victims[i] = uint32(vic[i])
	}
	for i := range p.groupPlaced {
		p.groupPlaced[i] = uint32(placed[i])
	}
	return p, nil
}

// expiredGangs is what expireGangs returns: per expired group and per forgotten pod, in the library's fixed order (groups in the caller's
// order, or ascending in ALL mode; inside a group the pods in ascending queue index).
type expiredGangs struct {
	group        []uint32 // the expired groups
	groupPods    []uint32 // waiting pods of the last pass forgotten for the group
	groupEarlier []uint32 // MatchedPodNodes entries of earlier cycles (no queue index): the shim takes those off their nodes itself
	pod          []uint32 // queue index of each forgotten pod
	node         []uint32 // the node it had been assumed on
}

// expireGangs: bs_seq_expire_flat — the shim's OnEvicted hook (controller.go:322-332) for the gangs whose PodNameUIDs entry ran out since
// the last seqPass: their waiting pods leave the nodes they were assumed on, matched returns to 0, and with deny the groups go onto the
// deny list (addToBackOff).  groups == nil with all: every gang that still has waiting pods.  P and G are the queue length and the group
// count of that pass (the result arrays' capacities).  It lives here and not beside seqPass in bsched_batch.go: the C11 client test
// requires go/c11_client/shim_client.c to call whatever that file calls.
func (g *gpuCore) expireGangs(groups []uint32, deny, all bool, P, G int) (*expiredGangs, error) {
	var flags C.uint32_t
	if deny {
		flags |= C.BS_SEQ_EXPIRE_DENY
	}
	var none C.uint32_t
	list, pList := u32s(groups)
	if all {
		flags |= C.BS_SEQ_EXPIRE_ALL
		list, pList = nil, nil
	} else if len(list) == 0 {
		pList = &none // an empty list is not NULL
	}
	gcap := len(list)
	if all {
		gcap = G
	}
	og, ogp, oge := make([]C.uint32_t, gcap+1), make([]C.uint32_t, gcap+1), make([]C.uint32_t, gcap+1)
	op, on := make([]C.uint32_t, P+1), make([]C.uint32_t, P+1)
	var counts [2]C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_seq_expire_flat(g.ctx, C.uint32_t(len(list)), pList, flags, C.uint32_t(gcap), &og[0], &ogp[0], &oge[0], C.uint32_t(P), &op[0], &on[0],
		&counts[0]); rc != C.BS_OK {
		return nil, fmt.Errorf("bs_seq_expire_flat: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	ng, np := int(counts[0]), int(counts[1])
	e := &expiredGangs{group: make([]uint32, ng), groupPods: make([]uint32, ng), groupEarlier: make([]uint32, ng), pod: make([]uint32, np), node: make([]uint32, np)}
	for i := 0; i < ng; i++ {
		e.group[i], e.groupPods[i], e.groupEarlier[i] = uint32(og[i]), uint32(ogp[i]), uint32(oge[i])
	}
	for i := 0; i < np; i++ {
		e.pod[i], e.node[i] = uint32(op[i]), uint32(on[i])
	}
	return e, nil
}

// droppedWaiters: the rows of the resident wait table that left with their nodes, in ascending id.
type droppedWaiters struct {
	n     uint32   // the true count (may exceed the rows asked for)
	id    []uint32 // the row's id: dead from now on
	node  []uint32 // the OLD index of the node it waited on
	group []int32  // its gang: matched of that group fell by one
}

// waitFollowNodes: bs_wait_nodes_apply — the resident wait table follows node-list surgery.  Called after the bs_nodes_apply call(s) it
// mirrors, with the kind and index fields of their deltas in order (the shim parks the last pass's waiting pods BEFORE the surgery); the
// bound table's bs_bound_nodes_apply takes the same two arrays, in either order.  Rows on removed nodes leave and come back here: the
// shim rejects those WaitingPods (or restores matched with bs_groups_apply to let the entry live to its TTL); every other row keeps its
// id and names its node by the new index.  rows: how many dropped rows to take back.  The shim has no resident wait cycle yet; when it
// gets one this is its step between the park and the next pass.
func (g *gpuCore) waitFollowNodes(kind, index []uint32, rows int) (*droppedWaiters, error) {
	if len(kind) != len(index) {
		return nil, fmt.Errorf("waitFollowNodes: %d kinds, %d indices", len(kind), len(index))
	}
	_, pKind := u32s(kind)
	_, pIndex := u32s(index)
	oid, onode, ogroup := make([]C.uint32_t, rows+1), make([]C.uint32_t, rows+1), make([]C.int32_t, rows+1)
	var n C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_wait_nodes_apply(g.ctx, C.uint32_t(len(kind)), pKind, pIndex, C.uint32_t(rows), &oid[0], &onode[0], &ogroup[0], &n); rc != C.BS_OK {
		return nil, fmt.Errorf("bs_wait_nodes_apply: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	k := int(n)
	if k > rows {
		k = rows
	}
	d := &droppedWaiters{n: uint32(n), id: make([]uint32, k), node: make([]uint32, k), group: make([]int32, k)}
	for i := 0; i < k; i++ {
		d.id[i], d.node[i], d.group[i] = uint32(oid[i]), uint32(onode[i]), int32(ogroup[i])
	}
	return d, nil
}

// boundRows: what bs_bound_bind reports for the rows it bound, in the call's order (wait rows first, then queue pods).
type boundRows struct {
	firstID uint32   // row i is bound-pod id firstID + i from now on
	node    []uint32 // the node each row bound on
}

// bindReleased: bs_bound_bind — the pods that leave Permit enter the resident bound table on the device.  The flat prototype is
//
//	int bs_bound_bind(bs_ctx*, uint32_t n_wait, const uint32_t* wait_id, uint32_t n_pod, const uint32_t* pod_index,
//	                  const int32_t* priority, const int64_t* start_ns, const uint8_t* pdb_violating, uint32_t* node_out, uint32_t* first_id_out)
//
// waitIDs: the wait-table ids of the released gangs' rows (the shim keys its WaitingPod map by them); podIndex: the queue indices of the
// pods the last seqPass placed and released.  priority, startNs and pdb are per row, the wait rows first; pdb may be nil.  Nodes, groups,
// request lanes and key bits are read where they are resident, the wait rows leave their table, node requests stay as the assume step left
// them.  In the cycle it stands between the pass and the park:
//
//	seqPass -> bindReleased(ids of the released gangs, placed pods) -> bs_wait_park -> bs_pods_apply (bound and parked pods leave the queue)
//
// and replaces bs_wait_release + marshalling + applyBoundEvents(moveNodes = false) for these pods.  The shim has no resident wait cycle
// yet; when it gets one this is its bind step.
func (g *gpuCore) bindReleased(waitIDs, podIndex []uint32, priority []int32, startNs []int64, pdb []uint8) (*boundRows, error) {
	n := len(waitIDs) + len(podIndex)
	if len(priority) != n || len(startNs) != n || (pdb != nil && len(pdb) != n) {
		return nil, fmt.Errorf("bindReleased: %d rows, %d priorities, %d start times, %d pdb bits", n, len(priority), len(startNs), len(pdb))
	}
	_, pWait := u32s(waitIDs)
	_, pPod := u32s(podIndex)
	_, pPrio := i32s(priority)
	start, bits, out := make([]C.int64_t, n+1), make([]C.uint8_t, n+1), make([]C.uint32_t, n+1)
	for i := 0; i < n; i++ {
		start[i] = C.int64_t(startNs[i])
		if pdb != nil {
			bits[i] = C.uint8_t(pdb[i])
		}
	}
	var pBits *C.uint8_t
	if pdb != nil {
		pBits = &bits[0]
	}
	var first C.uint32_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_bound_bind(g.ctx, C.uint32_t(len(waitIDs)), pWait, C.uint32_t(len(podIndex)), pPod, pPrio, &start[0], pBits, &out[0], &first); rc != C.BS_OK {
		return nil, fmt.Errorf("bs_bound_bind: %s (%s)", C.GoString(C.bs_strerror(rc)), C.GoString(C.bs_last_error(g.ctx)))
	}
	r := &boundRows{firstID: uint32(first), node: make([]uint32, n)}
	for i := 0; i < n; i++ {
		r.node[i] = uint32(out[i])
	}
	return r, nil
}
