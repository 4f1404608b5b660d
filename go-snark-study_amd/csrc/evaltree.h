// Index arithmetic of the evaluation-basis derivation (ecntt.hip, pk_derive_eval_impl): a node tree over the n nodes n+1 .. 2n with
// 2^L leaf slots, L = ceil(log2 n).  Leaf j < n is (x - x_j), the leaves above are the polynomial 1.  A node of level l (l = 0: the
// leaves, l = L: the root) with index b covers the leaf slots [b 2^l, (b + 1) 2^l); r of them are real, M_node is monic of degree r
// and the node carries a sequence of r points in a slot of 2^l (the rest of the slot is the point at infinity).
// The kernels and the host-compiled replay over Fr scalars (tests/host/evaltree_host_test.hip) share these functions.
#pragma once
#include <stdint.h>

#include "fp29.h"

namespace gs {

// number of real leaves below node b of level l
GS_HD uint32_t et_real(uint32_t n, int level, uint32_t b) {
  const uint64_t lo = (uint64_t)b << level, span = (uint64_t)1 << level;
  return lo >= n ? 0u : (uint32_t)(n - lo < span ? n - lo : span);
}
// first element of slot b of a buffer whose slots hold 2^slot_level elements (a node's own sequence: its level; its product: the
// parent's level)
GS_HD size_t et_slot(int slot_level, uint32_t b) { return (size_t)b << slot_level; }
// Child c (0 left, 1 right) of parent p: its sequence is the window [et_window(..), et_window(..) + et_real(child)) of
// c_parent * rev(M_sibling) -- the window starts at the sibling's degree.
GS_HD uint32_t et_child(uint32_t p, int c) { return 2 * p + (uint32_t)c; }
GS_HD uint32_t et_window(uint32_t n, int parent_level, uint32_t p, int c) { return et_real(n, parent_level - 1, et_child(p, c ^ 1)); }
// The product of child c of parent p lies in slot 2 p + c of a buffer whose slots have the PARENT's size 2^parent_level; the level's
// spectra (of the children's reversed polynomials, at that size) have the same layout, so the element a product element is multiplied
// by -- the SIBLING's spectrum at the same frequency -- is the one with the child bit flipped.
GS_HD size_t et_sibling_elem(int parent_level, size_t i) { return i ^ ((size_t)1 << parent_level); }

}  // namespace gs
