package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"math/big"
	"runtime"
	"unsafe"
)

// Compressed points: an x coordinate and a flag byte per point <-> a resident array of affine points (include/gosnark_hip.h,
// "compressed points").  Coordinates are 4 little-endian words in standard form, an Fq2 coordinate is c0 | c1.  The sign rule: y is
// the LARGER of {y, q - y} as canonical integers, in Fq2 decided by c1 and by c0 only when c1 = 0.  PointCodec holds the byte layouts of
// gnark, arkworks and the bn256 pairing crate, written down from those projects' sources from memory; no file written by any of them
// has been read (README, "Compressed points").

// Flag bits of one point.
const (
	PointLargestY = 1 // GS_POINT_LARGEST_Y
	PointInfinity = 2 // GS_POINT_INFINITY
)

func decompress(g2 bool, device int, x []uint64, flags []uint8) (Handle, []bool, error) {
	words := 4
	if g2 {
		words = 8
	}
	n := len(flags)
	if len(x) != words*n {
		return 0, nil, errors.New("gosnark-hip: one flag byte and 4 (G1) or 8 (G2) words per point")
	}
	ok := make([]uint8, n+1)
	var h C.gs_handle
	var bad, first C.uint64_t
	fb := append(flags[:n:n], 0) // a copy with one more byte: n = 0 still hands over readable memory
	fp := (*C.uint8_t)(unsafe.Pointer(&fb[0]))
	okp := (*C.uint8_t)(unsafe.Pointer(&ok[0]))
	err := onDevice(device, func() C.int {
		if g2 {
			return C.gs_g2_decompress(ptr(x), fp, C.size_t(n), &h, okp, &bad, &first)
		}
		return C.gs_g1_decompress(ptr(x), fp, C.size_t(n), &h, okp, &bad, &first)
	})
	runtime.KeepAlive(x)
	runtime.KeepAlive(fb)
	if err != nil {
		return 0, nil, err
	}
	out := make([]bool, n)
	for i := range out {
		out[i] = ok[i] != 0
	}
	return Handle(h), out, nil
}

// G1Decompress turns n x coordinates (4 words each) and n flag bytes into a resident G1 array on logical device `device`
// (gs_g1_decompress).  ok[i] is false for an entry that does not decode -- x >= q, x^3 + 3 not a square, an inconsistent flag -- and
// that entry is the point at infinity in the array; the call does not fail for it.  Call sequence = tests/c/point_codec.c.
func G1Decompress(device int, x []uint64, flags []uint8) (points Handle, ok []bool, err error) {
	return decompress(false, device, x, flags)
}

// G2Decompress is G1Decompress over the twist (8 words per x, c0 | c1; gs_g2_decompress).  The points are NOT tested for membership
// of the order-r subgroup: G2SubgroupCheck on the handle does that.
func G2Decompress(device int, x []uint64, flags []uint8) (points Handle, ok []bool, err error) {
	return decompress(true, device, x, flags)
}

func compress(g2 bool, points Handle, off, n int) ([]uint64, []uint8, error) {
	words := 4
	if g2 {
		words = 8
	}
	x, flags := make([]uint64, words*n), make([]uint8, n+1)
	fp := (*C.uint8_t)(unsafe.Pointer(&flags[0]))
	err := call(func() C.int {
		if g2 {
			return C.gs_g2_compress(C.gs_handle(points), C.size_t(off), C.size_t(n), ptr(x), fp)
		}
		return C.gs_g1_compress(C.gs_handle(points), C.size_t(off), C.size_t(n), ptr(x), fp)
	})
	if err != nil {
		return nil, nil, err
	}
	return x, flags[:n], nil
}

// G1Compress reads the points off .. off+n-1 of a resident G1 array as x coordinates and flag bytes (gs_g1_compress); a point at
// infinity gives x = 0 and PointInfinity.
func G1Compress(points Handle, off, n int) (x []uint64, flags []uint8, err error) {
	return compress(false, points, off, n)
}

// G2Compress is G1Compress for G2 arrays (gs_g2_compress).
func G2Compress(points Handle, off, n int) (x []uint64, flags []uint8, err error) {
	return compress(true, points, off, n)
}

// Meaning of a two-bit tag value.
const (
	TagSmaller = iota
	TagLarger
	TagInfinity
	TagInvalid
)

// PointCodec is a wire format of compressed points: the byte order of a coordinate, the order of the Fq2 halves, and what each value
// of the two most significant bits of the encoding's most significant byte means.
type PointCodec struct {
	BigEndian bool
	C1First   bool
	Tags      [4]int
}

// The three presets.  In Arkworks the tag sits in the LAST byte of the encoding.
var (
	Gnark        = PointCodec{true, true, [4]int{TagInvalid, TagInfinity, TagSmaller, TagLarger}}
	Bn256Pairing = PointCodec{true, true, [4]int{TagSmaller, TagInfinity, TagLarger, TagInvalid}}
	Arkworks     = PointCodec{false, false, [4]int{TagSmaller, TagInfinity, TagLarger, TagInvalid}}
)

// Decode turns n encodings of 32 (halves = 1) or 64 (halves = 2) bytes into the words and flag bytes G1Decompress / G2Decompress
// take.  An invalid tag becomes the flag value 4, which the device reports as a bad entry.
func (c PointCodec) Decode(buf []byte, halves int) (x []uint64, flags []uint8, err error) {
	size := 32 * halves
	if (halves != 1 && halves != 2) || len(buf)%size != 0 {
		return nil, nil, errors.New("gosnark-hip: compressed points are 32 (G1) or 64 (G2) bytes each")
	}
	n := len(buf) / size
	x, flags = make([]uint64, 4*halves*n), make([]uint8, n)
	flagOf := [4]uint8{0, PointLargestY, PointInfinity, 4}
	for i := 0; i < n; i++ {
		e := buf[size*i : size*(i+1)]
		top := 0
		if !c.BigEndian {
			top = size - 1
		}
		flags[i] = flagOf[c.Tags[e[top]>>6]]
		for h := 0; h < halves; h++ {
			src := h
			if halves == 2 && c.C1First {
				src = 1 - h
			}
			for k := 0; k < 32; k++ { // k = the byte's weight, 0 = least significant
				pos := 32*src + k
				if c.BigEndian {
					pos = 32*src + 31 - k
				}
				b := e[pos]
				if pos == top {
					b &= 0x3f
				}
				x[(4*halves)*i+4*h+k/8] |= uint64(b) << (8 * uint(k%8))
			}
		}
	}
	return x, flags, nil
}

// DecompressProofs turns n blobs of 128 bytes (A | B | C) into the proofs' points on logical device `device`: one G1Decompress call
// over the 2n points A and C, one G2Decompress call.  ok[i] is false when a point of proof i does not decode; that point is the point
// at infinity.
func DecompressProofs(device int, blobs [][]byte, c PointCodec) (a [][3]*big.Int, b [][3][2]*big.Int, cc [][3]*big.Int, ok []bool, err error) {
	n := len(blobs)
	g1, g2 := make([]byte, 0, 64*n), make([]byte, 0, 64*n)
	for _, p := range blobs {
		if len(p) != 128 {
			return nil, nil, nil, nil, errors.New("gosnark-hip: a compressed Groth16 proof is 128 bytes")
		}
		g1 = append(g1, p[:32]...)
		g2 = append(g2, p[32:96]...)
	}
	for _, p := range blobs {
		g1 = append(g1, p[96:]...)
	}
	x1, f1, err := c.Decode(g1, 1)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	x2, f2, err := c.Decode(g2, 2)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	h1, ok1, err := G1Decompress(device, x1, f1)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	defer Free(h1)
	h2, ok2, err := G2Decompress(device, x2, f2)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	defer Free(h2)
	p1, err := DownloadG1(h1, 2*n)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	b, err = DownloadG2(h2, n)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	ok = make([]bool, n)
	for i := range ok {
		ok[i] = ok1[i] && ok2[i] && ok1[n+i]
	}
	return p1[:n], b, p1[n:], ok, nil
}
