/* tests/mex_stub/mex.h plus the uint8 part of the Matrix API: what mex/bds_mex.c needs for its packed input ('acquire' with
 * iq = 2, a uint8 longSignal).  tests/test_packed_cases.py compiles the gateway with -DBDS_MEX_HAVE_UINT8 against this header. */
#ifndef BDS_TEST_MEX_STUB_PACKED_H
#define BDS_TEST_MEX_STUB_PACKED_H
#include "../mex_stub/mex.h"
bool mxIsUint8(const mxArray *a);
uint8_t *mxGetUint8s(const mxArray *a);
mxArray *mock_create_uint8(size_t n); /* 1 x n uint8 row (the stand-in's mxCreateNumericMatrix knows int8, int32 and double) */
#endif
