/* solve1_c64m_many.hip - the one-launch node solve (csrc/solve1_body.h) for many problems at once (hipsdp_solve_many): instance for
 * 64 < m <= 128; one workgroup per problem, the arguments in device memory */
#define S1_NCLS 64
#define S1_MBIG 1
#define S1_MANY
#define S1_KERNEL k_solve1_c64m_many
#define S1_LAUNCH_MANY hs_solve1_launch_c64m_many
#include "solve1_body.h"
