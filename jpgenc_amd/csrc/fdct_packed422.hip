// K1 for YUYV and UYVY (packed 4:2:2 groups; the order is a wave-uniform byte selector): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 8
#define JPGE_K1_ENTRY launch_fdct_packed422
#include "fdct.hip"
