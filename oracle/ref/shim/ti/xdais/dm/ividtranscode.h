/* ti/xdais/dm/ividtranscode.h -- stand-in for the host build of the reference
 * (oracle/ref): the names trik_vidtranscode_cv.h embeds as `base` members and
 * the two constants it uses.  The layouts are placeholders: nothing built
 * here reads a `base`, and the XDAIS function table that does is out of
 * scope. */
#ifndef TRIK_REF_SHIM_TI_XDAIS_DM_IVIDTRANSCODE_H_
#define TRIK_REF_SHIM_TI_XDAIS_DM_IVIDTRANSCODE_H_

#include <ti/xdais/ialg.h>

#define XDM_CUSTOMENUMBASE 0x100
#define IVIDTRANSCODE_MAXOUTSTREAMS 2

typedef struct IVIDTRANSCODE_Fxns {
  IALG_Fxns ialg;
} IVIDTRANSCODE_Fxns;

typedef struct IVIDTRANSCODE_Params {
  XDAS_Int32 size;
  XDAS_Int32 numOutputStreams;
  XDAS_Int32 formatInput;
  XDAS_Int32 formatOutput[IVIDTRANSCODE_MAXOUTSTREAMS];
} IVIDTRANSCODE_Params;

typedef struct IVIDTRANSCODE_DynamicParams {
  XDAS_Int32 size;
  XDAS_Int32 outputHeight[IVIDTRANSCODE_MAXOUTSTREAMS];
  XDAS_Int32 outputWidth[IVIDTRANSCODE_MAXOUTSTREAMS];
} IVIDTRANSCODE_DynamicParams;

typedef struct IVIDTRANSCODE_InArgs {
  XDAS_Int32 size;
} IVIDTRANSCODE_InArgs;

typedef struct IVIDTRANSCODE_OutArgs {
  XDAS_Int32 size;
} IVIDTRANSCODE_OutArgs;

#endif /* TRIK_REF_SHIM_TI_XDAIS_DM_IVIDTRANSCODE_H_ */
