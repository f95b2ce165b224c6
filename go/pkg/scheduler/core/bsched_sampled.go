// +build cgo

/*
Upstream's node sampling in the sequential pass (include/bsched.h "upstream's node sampling and rotating start", rule F; INTEGRATION.md,
"Which nodes are scored"): genericScheduler.findNodesThatFit starts at nextStartNodeIndex, stops once numFeasibleNodesToFind feasible nodes
are found and scores those only.  The library's context keeps no cursor between passes, as upstream's cursor lives in the scheduler and
not in the snapshot: sampleCursor is that field.  It is handed to every sampled pass as `start` and replaced by the pass's next_start
(bs_seq_sample_read).  Nothing here is compiled in this repository's image (no Go toolchain); the calls' behaviour is pinned by
tests/test_gpu_seq_sampled.py through the same entry points, which take flat arguments only.
*/
package core

/*
#include "bsched.h"
*/
import "C"

import "fmt"

// sampleCursor is nextStartNodeIndex and percentageOfNodesToScore of the scheduler this core serves.  The zero value is upstream's: cursor
// 0, the adaptive percentage.
type sampleCursor struct {
	next       uint32 // the cursor the next pass starts at; any value is valid, the pass takes it mod the node count
	percentage int32  // percentageOfNodesToScore; 0 or less: the adaptive default (50 - nodes/125, at least 5)
}

// numToFind: upstream's numFeasibleNodesToFind for a list of `nodes` nodes (bs_seq_sample_size, D9): pure arithmetic, no context.
func (s *sampleCursor) numToFind(nodes int) uint32 {
	return uint32(C.bs_seq_sample_size(C.uint32_t(nodes), C.int32_t(s.percentage)))
}

// sampledResult is what a sampled pass reports on top of seqResult: per queue pod the chosen node's total, the candidates kept (at most
// numToFind), the cursor its walk began at and the nodes it visited; 0 where the pod did not reach the node choice.
type sampledResult struct {
	total, nFit, start, visited []uint32
}

// readSampled: bs_seq_score_read and bs_seq_sample_read behind a sampled pass; the cursor behind the last pod goes into cur.  The caller
// holds g.mu.
func (g *gpuCore) readSampled(P int, cur *sampleCursor) (*sampledResult, error) {
	ct, cf, cs, cv := make([]C.uint32_t, P+1), make([]C.uint32_t, P+1), make([]C.uint32_t, P+1), make([]C.uint32_t, P+1)
	if rc := C.bs_seq_score_read(g.ctx, C.uint32_t(P), &ct[0], &cf[0]); rc != C.BS_OK {
		return nil, g.pdbErr("bs_seq_score_read", rc)
	}
	var next C.uint32_t
	if rc := C.bs_seq_sample_read(g.ctx, C.uint32_t(P), &cs[0], &cv[0], &next); rc != C.BS_OK {
		return nil, g.pdbErr("bs_seq_sample_read", rc)
	}
	cur.next = uint32(next) // the hand-over: the next cycle's pass starts where this one's last walk ended
	s := &sampledResult{total: make([]uint32, P), nFit: make([]uint32, P), start: make([]uint32, P), visited: make([]uint32, P)}
	for i := 0; i < P; i++ {
		s.total[i], s.nFit[i], s.start[i], s.visited[i] = uint32(ct[i]), uint32(cf[i]), uint32(cs[i]), uint32(cv[i])
	}
	return s, nil
}

// seqPassScoredSampled: seqPass with the scored node choice over a sample of the nodes (bs_seq_run_scored_sampled, rule F over rule P):
// every pod's walk starts at a cursor that rotates from pod to pod, stops behind numToFind candidates and scores those; ties go to the
// node visited first.  P is the resident queue's length, nodes the node list's.  cur is read for the pass's first cursor and written with
// the cursor behind its last pod.
func (g *gpuCore) seqPassScoredSampled(w scoreWeights, cur *sampleCursor, P, nodes int) (*seqResult, *sampledResult, error) {
	cap := g.groups + 1
	r := &seqResult{pfCode: make([]C.uint8_t, P+1), podNode: make([]C.int32_t, P+1), releasedGroup: make([]C.uint32_t, cap),
		releasedPods: make([]C.uint32_t, cap), readyNs: make([]C.int64_t, cap), lastPermitted: make([]C.uint8_t, P+1)}
	firstNs := make([]C.int64_t, cap)
	var scalars [8]C.int64_t
	g.mu.Lock()
	defer g.mu.Unlock()
	if rc := C.bs_seq_run_scored_sampled_flat(g.ctx, C.uint32_t(C.BS_STAGE_PREFILTER), C.uint32_t(w.least), C.uint32_t(w.most),
		C.uint32_t(w.balanced), C.uint32_t(cur.numToFind(nodes)), C.uint32_t(cur.next), &r.pfCode[0], nil, nil, &r.podNode[0], C.uint32_t(cap),
		&r.releasedGroup[0], &r.releasedPods[0], &firstNs[0], &r.readyNs[0], &scalars[0], &r.lastPermitted[0]); rc != C.BS_OK {
		return nil, nil, g.pdbErr("bs_seq_run_scored_sampled_flat", rc)
	}
	r.nReleased = int(scalars[0])
	s, err := g.readSampled(P, cur)
	if err != nil {
		return nil, nil, err
	}
	return r, s, nil
}

// seqPassScoredNominatedSampled: seqPassScoredNominated over a sample of the nodes (bs_seq_run_scored_nominated_sampled, rule F over rule
// SP): the pass a nominating cycle of a cluster with default settings ends in.  priority, ownRow and `consumed` are
// seqPassScoredNominated's; cur as in seqPassScoredSampled.
func (g *gpuCore) seqPassScoredNominatedSampled(w scoreWeights, cur *sampleCursor, priority []int32, ownRow []uint32, nodes int) (r *seqResult,
	consumed []consumedNominee, s *sampledResult, err error) {
	P := len(priority)
	if ownRow != nil && len(ownRow) != P {
		return nil, nil, nil, fmt.Errorf("seqPassScoredNominatedSampled: %d own rows for %d pods", len(ownRow), P)
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
	if rc := C.bs_seq_run_scored_nominated_sampled_flat(g.ctx, C.uint32_t(C.BS_STAGE_PREFILTER), C.uint32_t(P), &prio[0], &own[0],
		C.uint32_t(w.least), C.uint32_t(w.most), C.uint32_t(w.balanced), C.uint32_t(cur.numToFind(nodes)), C.uint32_t(cur.next), &r.pfCode[0], nil,
		nil, &r.podNode[0], C.uint32_t(cap), &r.releasedGroup[0], &r.releasedPods[0], &firstNs[0], &r.readyNs[0], &scalars[0],
		&r.lastPermitted[0]); rc != C.BS_OK {
		return nil, nil, nil, g.pdbErr("bs_seq_run_scored_nominated_sampled_flat", rc)
	}
	r.nReleased = int(scalars[0])
	if s, err = g.readSampled(P, cur); err != nil {
		return nil, nil, nil, err
	}
	var n C.uint32_t
	if rc := C.bs_seq_nominated_read(g.ctx, 0, nil, nil, nil, &n); rc != C.BS_OK {
		return nil, nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	if n == 0 {
		return r, nil, s, nil
	}
	id, pod, node := make([]C.uint32_t, n), make([]C.uint32_t, n), make([]C.uint32_t, n)
	if rc := C.bs_seq_nominated_read(g.ctx, n, &id[0], &pod[0], &node[0], &n); rc != C.BS_OK {
		return nil, nil, nil, g.pdbErr("bs_seq_nominated_read", rc)
	}
	consumed = make([]consumedNominee, n)
	for i := range consumed {
		consumed[i] = consumedNominee{uint32(id[i]), uint32(pod[i]), uint32(node[i])}
	}
	return r, consumed, s, nil
}
