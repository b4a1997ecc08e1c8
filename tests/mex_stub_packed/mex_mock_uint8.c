/* The stand-in for the MEX runtime of tests/mex_stub/mex_mock.c (TEST INFRASTRUCTURE), with uint8 arrays added: the same
 * translation unit -- its array struct is private to it -- and one more class. */
#include "mex.h"

#include "../mex_stub/mex_mock.c"

enum { C_UINT8 = C_LOGICAL + 1 }; /* (elsize: 1 byte, like every class the table there does not name) */

bool mxIsUint8(const mxArray *a) { return a && a->cls == C_UINT8; }
uint8_t *mxGetUint8s(const mxArray *a) { return a && a->cls == C_UINT8 ? (uint8_t *)a->data : NULL; }
mxArray *mock_create_uint8(size_t n) { return make(C_UINT8, 1, n); }
