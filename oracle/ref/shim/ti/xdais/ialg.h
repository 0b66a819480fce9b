/* ti/xdais/ialg.h -- stand-in for the host build of the reference
 * (oracle/ref).  The algorithm classes never look inside these types; the
 * XDAIS function table that does (vidtranscode_cv_fxns.c) is not built. */
#ifndef TRIK_REF_SHIM_TI_XDAIS_IALG_H_
#define TRIK_REF_SHIM_TI_XDAIS_IALG_H_

#include <ti/xdais/xdas.h>

#define IALG_EOK   (0)
#define IALG_EFAIL (-1)

typedef struct IALG_Fxns {
  Void* implementationId;
} IALG_Fxns;

typedef struct IALG_Obj {
  struct IALG_Fxns* fxns;
} IALG_Obj;

typedef struct IALG_Obj* IALG_Handle;

#endif /* TRIK_REF_SHIM_TI_XDAIS_IALG_H_ */
