// K1 for NV16 (Y plane + a plane of interleaved Cb,Cr rows at half width): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 9
#define JPGE_K1_ENTRY launch_fdct_nv16
#include "fdct.hip"
