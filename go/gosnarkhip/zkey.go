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

// circuit.zkey: the binary key file circom / snarkjs write today.  Its sections go to the device as they lie in the file (a
// memory-mapped file is fine: nothing here turns a coordinate into a big.Int) and are converted there.  A zkey has no C matrix --
// the R1CS handle is a product system, c_j = a_j b_j on the domain -- and no hExps: section 9 is the coset evaluation basis, so the
// key is coset-only and proves through the witness entry points (ProveWitness, ProveWitnessBegin, the host-buffer tickets) alone.
// The container itself (magic, section table) is the caller's to walk; go-snark-study_amd/circom.py documents the layout.

func bytePtr(b []byte) *byte {
	if len(b) == 0 {
		return nil
	}
	return &b[0]
}

// UploadG1AffineMont makes n = len(b)/64 G1 points in the zkey encoding (x | y, each 32 little-endian bytes of value * 2^256 mod q,
// all zero = infinity) resident on logical device `device` (gs_g1_upload_affine_mont).
func UploadG1AffineMont(device int, b []byte) (Handle, error) {
	if len(b)%64 != 0 {
		return 0, errors.New("gosnark-hip: G1 points of a zkey are 64 bytes each")
	}
	var h C.gs_handle
	err := onDevice(device, func() C.int { return C.gs_g1_upload_affine_mont(unsafe.Pointer(bytePtr(b)), C.size_t(len(b)/64), &h) })
	runtime.KeepAlive(b)
	return Handle(h), err
}

// UploadG2AffineMont is UploadG1AffineMont for G2 (x.c0 | x.c1 | y.c0 | y.c1, 128 bytes a point; gs_g2_upload_affine_mont).
func UploadG2AffineMont(device int, b []byte) (Handle, error) {
	if len(b)%128 != 0 {
		return 0, errors.New("gosnark-hip: G2 points of a zkey are 128 bytes each")
	}
	var h C.gs_handle
	err := onDevice(device, func() C.int { return C.gs_g2_upload_affine_mont(unsafe.Pointer(bytePtr(b)), C.size_t(len(b)/128), &h) })
	runtime.KeepAlive(b)
	return Handle(h), err
}

// UploadR1CSZkey builds the CSR arrays of A and B on the device from the 44-byte records of section 4 (without the count word in
// front of them) and keeps them resident as a product system over the domain of 2^log2Domain points (gs_r1cs_upload_zkey).
func UploadR1CSZkey(device, log2Domain, nvars int, coefs []byte) (*R1CS, error) {
	if len(coefs)%44 != 0 {
		return nil, errors.New("gosnark-hip: coefficient records of a zkey are 44 bytes each")
	}
	var h C.gs_handle
	err := onDevice(device, func() C.int {
		return C.gs_r1cs_upload_zkey(C.size_t(log2Domain), C.size_t(nvars), unsafe.Pointer(bytePtr(coefs)), C.size_t(len(coefs)/44), &h)
	})
	runtime.KeepAlive(coefs)
	if err != nil {
		return nil, err
	}
	return &R1CS{Handle(h), 1 << uint(log2Domain), nvars}, nil
}

// ZkeySections are the payloads of a circuit.zkey a prover needs, as bytes of the file.  C is section 8 with (NPublic + 1) * 64 zero
// bytes in front (the file leaves the public signals out); Alpha1 .. Delta2 are cut out of section 2.
type ZkeySections struct {
	A, B1, B2, C, H       []byte
	Alpha1, Beta1, Delta1 []byte // 64 bytes each
	Beta2, Delta2         []byte // 128 bytes each
	Log2Domain            int
	NVars, NPublic        int
}

// one point of the header -> its Jacobian limbs, by way of the device (the conversion lives there)
func singleG1(device int, b []byte, dst []uint64) error {
	h, err := UploadG1AffineMont(device, b)
	if err != nil {
		return err
	}
	defer Free(h)
	return call(func() C.int { return C.gs_g1_download(C.gs_handle(h), ptr(dst), 1) })
}

func singleG2(device int, b []byte, dst []uint64) error {
	h, err := UploadG2AffineMont(device, b)
	if err != nil {
		return err
	}
	defer Free(h)
	return call(func() C.int { return C.gs_g2_download(C.gs_handle(h), ptr(dst), 1) })
}

// NewGroth16KeyZkey assembles the coset-only key of a zkey on logical device `device`: 5 x gs_g*_upload_affine_mont,
// gs_groth16_pk_create_domain, 5 x gs_free.  Call sequence = tests/c/zkey_prove.c.
func NewGroth16KeyZkey(device int, p ZkeySections) (*Groth16Key, error) {
	if len(p.Alpha1) != 64 || len(p.Beta1) != 64 || len(p.Delta1) != 64 || len(p.Beta2) != 128 || len(p.Delta2) != 128 {
		return nil, errors.New("gosnark-hip: the single points of a zkey header are 64 (G1) and 128 (G2) bytes")
	}
	var hs [5]Handle
	defer func() {
		for _, h := range hs {
			_ = Free(h)
		}
	}()
	var err error
	for i, b := range [][]byte{p.A, p.B1, nil, p.C, p.H} {
		if i == 2 {
			hs[i], err = UploadG2AffineMont(device, p.B2)
		} else {
			hs[i], err = UploadG1AffineMont(device, b)
		}
		if err != nil {
			return nil, err
		}
	}
	singles1 := make([]uint64, 36)
	singles2 := make([]uint64, 48)
	for i, b := range [][]byte{p.Alpha1, p.Beta1, p.Delta1} {
		if err = singleG1(device, b, singles1[12*i:12*i+12]); err != nil {
			return nil, err
		}
	}
	for i, b := range [][]byte{p.Beta2, p.Delta2} {
		if err = singleG2(device, b, singles2[24*i:24*i+24]); err != nil {
			return nil, err
		}
	}
	var h C.gs_handle
	err = call(func() C.int {
		return C.gs_groth16_pk_create_domain(C.gs_handle(hs[0]), C.gs_handle(hs[1]), C.gs_handle(hs[2]), C.gs_handle(hs[3]), C.gs_handle(hs[4]),
			ptr(singles1[0:]), ptr(singles1[12:]), ptr(singles1[24:]), ptr(singles2[0:]), ptr(singles2[24:]),
			C.size_t(p.Log2Domain), C.size_t(p.NVars), C.size_t(p.NPublic), &h)
	})
	runtime.KeepAlive(singles1)
	runtime.KeepAlive(singles2)
	if err != nil {
		return nil, err
	}
	return &Groth16Key{Handle(h), p.NVars, p.NPublic}, nil
}
