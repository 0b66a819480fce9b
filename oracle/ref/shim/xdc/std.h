/* xdc/std.h -- stand-in for the host build of the reference (oracle/ref):
 * the fixed-width integer names the algorithm headers rely on. */
#ifndef TRIK_REF_SHIM_XDC_STD_H_
#define TRIK_REF_SHIM_XDC_STD_H_

#include <stddef.h>
#include <stdint.h>

typedef signed char    Int8;
typedef unsigned char  Uint8;
typedef short          Int16;
typedef unsigned short Uint16;
typedef int            Int32;
typedef unsigned int   Uint32;
typedef int            Int;
typedef unsigned int   Uns;
typedef void           Void;
typedef void*          Ptr;

#endif /* TRIK_REF_SHIM_XDC_STD_H_ */
