// sk_sdtwq_hint.hip -- the tagged screening sweep and the hinted pre-roll (k_sdtw_qh / k_sdtw_ph: the bodies of
// sk_sdtwq.hip with HINT = true, int16 feed, 8 and 16 lanes per read); a translation unit of its own so that it builds
// beside the three feeds.
#define SK_SDTWQ_FEED 0
#define SK_SDTWQ_HINT 1
#include "sk_sdtwq.hip"
