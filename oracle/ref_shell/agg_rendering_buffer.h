// TEST INFRASTRUCTURE: stands in for the AGG header of this name (see agg_shell.h).
#include "agg_shell.h"
