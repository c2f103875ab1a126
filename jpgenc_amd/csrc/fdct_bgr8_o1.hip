// K1 for BGR8, oriented, source rows forwards or backwards, columns as they are (JPGE_ORIENT_FLIP_V): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 1
#define JPGE_K1_ORIENT 1
#define JPGE_K1_ENTRY launch_fdct_bgr8_o1
#include "fdct.hip"
