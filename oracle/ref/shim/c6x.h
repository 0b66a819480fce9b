/*
 * c6x.h -- stand-in for TI's C6000 intrinsics header, for the host build of
 * the reference (oracle/ref/Makefile).  TEST INFRASTRUCTURE ONLY.
 *
 * The reference's algorithm headers use 23 C64x+ intrinsics.  Twenty of them
 * map onto the emulations of oracle/trik_oracle.c (trik_c64x_*, written from
 * TI's published intrinsic definitions and held by the known-answer tests of
 * tests/test_oracle.py), so that there is one definition of each; _loll,
 * _hill and _itoll are register moves and are written inline here.
 */
#ifndef TRIK_REF_SHIM_C6X_H_
#define TRIK_REF_SHIM_C6X_H_

#include <stddef.h>
#include <stdint.h>

#include "trik_oracle.h"

#define _add2    trik_c64x_add2
#define _shr2    trik_c64x_shr2
#define _pack2   trik_c64x_pack2
#define _packh2  trik_c64x_packh2
#define _packlh2 trik_c64x_packlh2
#define _packhl2 trik_c64x_packhl2
#define _packh4  trik_c64x_packh4
#define _spacku4 trik_c64x_spacku4
#define _unpklu4 trik_c64x_unpklu4
#define _unpkhu4 trik_c64x_unpkhu4
#define _maxu4   trik_c64x_maxu4
#define _minu4   trik_c64x_minu4
#define _cmpeq2  trik_c64x_cmpeq2
#define _cmpltu4 trik_c64x_cmpltu4
#define _cmpgtu4 trik_c64x_cmpgtu4
#define _dotpn2  trik_c64x_dotpn2
#define _dotpus4 trik_c64x_dotpus4
#define _mpyu4ll trik_c64x_mpyu4ll
#define _clr     trik_c64x_clr
#define _swap4   trik_c64x_swap4

static inline uint32_t _loll(uint64_t v) { return (uint32_t)v; }
static inline uint32_t _hill(uint64_t v) { return (uint32_t)(v >> 32); }
static inline uint64_t _itoll(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

#endif /* TRIK_REF_SHIM_C6X_H_ */
