// Host stand-in for <hip/hip_runtime.h>: lets g++ compile sos_amd/csrc/ldbl.h (tests only).
#define __device__
#define __forceinline__ inline
