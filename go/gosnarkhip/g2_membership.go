package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

// G2 subgroup membership of whole arrays.  The twist E'(Fq2) has the cofactor 2q - r = 10069 x (a 246-bit number), the uploads test the
// curve equation only, and the random linear combinations of CheckPtau, CheckLagrangeLevelsG2 and CheckKey let a point that is off the
// order-r subgroup by an element of order 10069 through about once in 10069 challenges.  A section of unknown origin goes through
// G2SubgroupCheck first; include/gosnark_hip.h has the formula and why no linear combination can replace the per-point test.

// NoBadPoint is the index G2SubgroupCheck returns when every point tested is in the subgroup.
const NoBadPoint = ^uint64(0)

// G2SubgroupCheck tests the points off .. off+n-1 of a resident G2 array (gs_g2_subgroup_check): nbad = how many lie outside the
// order-r subgroup, firstBad = the smallest index of one, counted from the start of the array, or NoBadPoint.  The point at infinity
// is a member; n = 0 is legal.  Exact and per point; it builds no window table.  Call sequence = tests/c/g2_membership.c.
func G2SubgroupCheck(points Handle, off, n int) (nbad, firstBad uint64, err error) {
	var bad, first C.uint64_t
	err = call(func() C.int { return C.gs_g2_subgroup_check(C.gs_handle(points), C.size_t(off), C.size_t(n), &bad, &first) })
	if err != nil {
		return 0, NoBadPoint, err
	}
	return uint64(bad), uint64(first), nil
}
