/* ti/xdais/xdas.h -- stand-in for the host build of the reference
 * (oracle/ref): the XDAS_* scalar types.  XDAS_Int8 is signed char because
 * the algorithm headers assign XDAS_Int8* image pointers to int8_t*. */
#ifndef TRIK_REF_SHIM_TI_XDAIS_XDAS_H_
#define TRIK_REF_SHIM_TI_XDAIS_XDAS_H_

#include <xdc/std.h>

typedef Void   XDAS_Void;
typedef Uint8  XDAS_Bool;
typedef Int8   XDAS_Int8;
typedef Uint8  XDAS_UInt8;
typedef Int16  XDAS_Int16;
typedef Uint16 XDAS_UInt16;
typedef Int32  XDAS_Int32;
typedef Uint32 XDAS_UInt32;

#define XDAS_TRUE  1
#define XDAS_FALSE 0

#endif /* TRIK_REF_SHIM_TI_XDAIS_XDAS_H_ */
