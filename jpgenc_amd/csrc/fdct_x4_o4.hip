// K1 for 4-byte pixels (RGBA8, BGRA8), oriented, transposed and mirrored (JPGE_ORIENT_TRANSVERSE, _ROT270): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 2
#define JPGE_K1_ORIENT 4
#define JPGE_K1_ENTRY launch_fdct_x4_o4
#include "fdct.hip"
