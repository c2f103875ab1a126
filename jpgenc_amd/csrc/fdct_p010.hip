// K1 for P010 (10-bit 4:2:0 in 16-bit words: Y plane + interleaved Cb,Cr plane at half size): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 11
#define JPGE_K1_ENTRY launch_fdct_p010
#include "fdct.hip"
