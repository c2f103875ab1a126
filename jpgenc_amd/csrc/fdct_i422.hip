// K1 for I422 (Y, Cb, Cr planes, chroma at half width): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 10
#define JPGE_K1_ENTRY launch_fdct_i422
#include "fdct.hip"
