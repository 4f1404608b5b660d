package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"
)

// Groth16 setup from a powers-of-tau transcript: nobody knows tau, so the Lagrange bases of the domain and the per-signal arrays of a
// circuit.zkey are computed on points.  The transcript's sections go to the device as they lie in the .ptau file (UploadG1AffineMont /
// UploadG2AffineMont), the circuit as a domain R1CS with the rows nConstraints + s = (signal s, 1) appended to A (UploadR1CSDomain);
// go-snark-study_amd/circom.py (SetupFromPtau, ContributeDelta) documents the file layouts and the order of the calls.

// LagrangeG1 is the inverse transform of the 2^log2N points of `powers` from index `off`, carried out in the group
// (gs_g1_lagrange): out[j] = (1/n) sum_i w^(-ij) P[off+i].  With oddHalf it is the odd entries of the transform of twice the size
// (2n - 1 or 2n points from off; a missing last point is the point at infinity): the coset evaluation basis of a zkey.
func LagrangeG1(powers Handle, off, log2N int, oddHalf bool) (Handle, error) {
	var h C.gs_handle
	var odd C.int
	if oddHalf {
		odd = 1
	}
	err := call(func() C.int { return C.gs_g1_lagrange(C.gs_handle(powers), C.size_t(off), C.size_t(log2N), odd, &h) })
	return Handle(h), err
}

// LagrangeG2 is LagrangeG1 without oddHalf for G2 points (gs_g2_lagrange).
func LagrangeG2(powers Handle, off, log2N int) (Handle, error) {
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g2_lagrange(C.gs_handle(powers), C.size_t(off), C.size_t(log2N), &h) })
	return Handle(h), err
}

// ColumnSumsG1 gives out[s] = sum_j a_js Ba[j] + b_js Bb[j] + c_js Bc[j] for every variable s of a resident R1CS
// (gs_r1cs_colsum_g1); a basis handle of 0 leaves its matrix out.
func (r *R1CS) ColumnSumsG1(basisA, basisB, basisC Handle) (Handle, error) {
	var h C.gs_handle
	err := call(func() C.int {
		return C.gs_r1cs_colsum_g1(C.gs_handle(r.h), C.gs_handle(basisA), C.gs_handle(basisB), C.gs_handle(basisC), &h)
	})
	return Handle(h), err
}

// ColumnSumsG2 is ColumnSumsG1 over G2 bases (gs_r1cs_colsum_g2).
func (r *R1CS) ColumnSumsG2(basisA, basisB, basisC Handle) (Handle, error) {
	var h C.gs_handle
	err := call(func() C.int {
		return C.gs_r1cs_colsum_g2(C.gs_handle(r.h), C.gs_handle(basisA), C.gs_handle(basisB), C.gs_handle(basisC), &h)
	})
	return Handle(h), err
}

// ScaleG1 gives out[i] = k P[i] for the four limbs of k (gs_g1_scale): a phase-2 contribution multiplies C and H by 1 / delta.
func ScaleG1(bases Handle, k []uint64) (Handle, error) {
	if len(k) != 4 {
		return 0, errors.New("gosnark-hip: a scalar is four 64-bit limbs")
	}
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g1_scale(C.gs_handle(bases), ptr(k), &h) })
	runtime.KeepAlive(k)
	return Handle(h), err
}

// DownloadG1AffineMont writes the first len(out)/64 points of a G1 base array in the zkey encoding (gs_g1_download_affine_mont);
// out may be a memory-mapped section of the output file.
func DownloadG1AffineMont(bases Handle, out []byte) error {
	if len(out)%64 != 0 {
		return errors.New("gosnark-hip: G1 points of a zkey are 64 bytes each")
	}
	err := call(func() C.int {
		return C.gs_g1_download_affine_mont(C.gs_handle(bases), unsafe.Pointer(bytePtr(out)), C.size_t(len(out)/64))
	})
	runtime.KeepAlive(out)
	return err
}

// DownloadG2AffineMont is DownloadG1AffineMont for G2 (128 bytes a point; gs_g2_download_affine_mont).
func DownloadG2AffineMont(bases Handle, out []byte) error {
	if len(out)%128 != 0 {
		return errors.New("gosnark-hip: G2 points of a zkey are 128 bytes each")
	}
	err := call(func() C.int {
		return C.gs_g2_download_affine_mont(C.gs_handle(bases), unsafe.Pointer(bytePtr(out)), C.size_t(len(out)/128))
	})
	runtime.KeepAlive(out)
	return err
}

// ZkeyArrays are the array sections of a circuit.zkey with delta = 1, resident: A, B1, C-with-IC (K: the signals 0 .. nPublic are IC,
// the rest is C), H in G1 and B2 in G2.
type ZkeyArrays struct {
	A, B1, B2, K, H Handle
}

// SetupZkeyArrays computes them from the transcript's resident sections (tauG1 with at least 2^(log2Domain+1) - 1 points, the others
// with 2^log2Domain) and the circuit's domain R1CS: 5 x gs_g*_lagrange, 4 x gs_r1cs_colsum_g*, 4 x gs_free.  Call sequence =
// tests/c/zkey_setup.c.
func SetupZkeyArrays(r *R1CS, tauG1, tauG2, alphaTauG1, betaTauG1 Handle, log2Domain int) (*ZkeyArrays, error) {
	var z ZkeyArrays
	var l, l2, la, lb Handle
	defer func() {
		for _, h := range []Handle{l, l2, la, lb} {
			if h != 0 {
				_ = Free(h)
			}
		}
	}()
	var err error
	if l, err = LagrangeG1(tauG1, 0, log2Domain, false); err != nil {
		return nil, err
	}
	if z.H, err = LagrangeG1(tauG1, 0, log2Domain, true); err != nil {
		return nil, err
	}
	if l2, err = LagrangeG2(tauG2, 0, log2Domain); err != nil {
		return nil, err
	}
	if la, err = LagrangeG1(alphaTauG1, 0, log2Domain, false); err != nil {
		return nil, err
	}
	if lb, err = LagrangeG1(betaTauG1, 0, log2Domain, false); err != nil {
		return nil, err
	}
	if z.A, err = r.ColumnSumsG1(l, 0, 0); err != nil {
		return nil, err
	}
	if z.B1, err = r.ColumnSumsG1(0, l, 0); err != nil {
		return nil, err
	}
	if z.B2, err = r.ColumnSumsG2(0, l2, 0); err != nil {
		return nil, err
	}
	if z.K, err = r.ColumnSumsG1(lb, la, l); err != nil {
		return nil, err
	}
	return &z, nil
}
