// K1 for 4-byte pixels (RGBA8, BGRA8): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 2
#define JPGE_K1_ENTRY launch_fdct_x4
#include "fdct.hip"
