// Preprocessed by the Makefile (never compiled): "@ <prefix> <NV>_<MD>_<W> ..." for every family of PINKHIP_FAMILIES, on
// the last line of the output -- what its objects are named after.
#include "dispatch.h"
#define PINKHIP_ROW_(NV, MD, W) NV##_##MD##_##W
#define PINKHIP_ROW(NV, MD, W) PINKHIP_ROW_(NV, MD, W)
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) @ PREFIX TABLE(PINKHIP_ROW)
PINKHIP_FAMILIES(PINKHIP_FAMILY)
