// bs_pdb.hpp — resident PodDisruptionBudgets (include/bsched.h, bs_pdb_load / bs_pdb_members_append / bs_pdb_allowed_apply): the PDB bit
// of every bound pod follows the budgets' status on the device.  Which PDBs select a pod is string work the caller does once, when the pod
// binds; it arrives as a CSR by bound-pod id (moff / member).  Whether a PDB is exhausted is one int32 per PDB (allowed).  The bit of the
// entry with id i is any(allowed[m] <= 0 for m in member[moff[i] .. moff[i + 1])), and an id at or beyond `covered` has no PDB.
//
// Two launches (plain loads and stores, no LDS, no atomics; the hand-over between them is the launch boundary):
//   k_pdb_allowed  one thread per (index, value) pair of the staged blob: allowed[index] = value (the host refused a repeated index).
//   k_pdb_bits     one wave per node, four per workgroup (the shape of k_bn_move / k_ba_merge): lanes stride over the node's list, 64
//                  entries per step; a lane loads its entry's id and the id's two offsets and walks its member run — short, divergent —
//                  ORing allowed[m] <= 0 (signed).  One byte store per lane, coalesced across the wave; the step's ballot is counted, and
//                  lane 0 stores the node's violating count.  A node with an empty list stores a zero count.  Only live entries are
//                  visited: the walk goes through the table, so the rows of dead ids are never read.
// Neither kernel depends on the scalar-lane count, so they are no templates: tu_bound.hip alone emits them (a unity build includes it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bs {

struct PdbDev {
  // the live table: the CSR by node, the id column; the two columns the recompute rewrites in place
  const uint32_t* boff;     // [n + 1]
  const uint32_t* bid;
  uint8_t* bpdb;
  uint32_t* bnviol;         // [n]
  uint32_t n;
  // the resident PDB state
  const uint32_t* moff;     // [covered + 1]
  const uint32_t* member;   // [moff[covered]], every value < the PDB count
  int32_t* allowed;         // [PDB count]
  uint32_t covered;
  // bs_pdb_allowed_apply's pairs (pinned host memory, read in place)
  const uint32_t* index;
  const int32_t* value;
  uint32_t count;
};

__global__ __launch_bounds__(256) void k_pdb_allowed(PdbDev a) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < a.count) a.allowed[a.index[t]] = a.value[t];
}

__global__ __launch_bounds__(256) void k_pdb_bits(PdbDev a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= a.n) return;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k]);
  const uint32_t b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k + 1]);
  uint32_t viol = 0;
  for (uint32_t base = b0; base < b1; base += 64u) {
    const uint32_t j = base + lane;
    bool bit = false;
    if (j < b1) {
      const uint32_t i = a.bid[j];
      if (i < a.covered) {
        const uint32_t m1 = a.moff[i + 1];
        for (uint32_t x = a.moff[i]; x < m1; ++x) bit |= a.allowed[a.member[x]] <= 0;
      }
      a.bpdb[j] = bit ? (uint8_t)1 : (uint8_t)0;
    }
    viol += (uint32_t)__builtin_popcountll(__ballot(bit));
  }
  if (lane == 0) a.bnviol[k] = viol;
}

}  // namespace bs
