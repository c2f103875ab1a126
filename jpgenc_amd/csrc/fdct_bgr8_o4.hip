// K1 for BGR8, oriented, transposed and mirrored (JPGE_ORIENT_TRANSVERSE, _ROT270): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 1
#define JPGE_K1_ORIENT 4
#define JPGE_K1_ENTRY launch_fdct_bgr8_o4
#include "fdct.hip"
