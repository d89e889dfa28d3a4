/* The sender includes the Morse table under a spelling that exists only on a case-insensitive file system; this forwards it to the
 * file as it is spelled (found through an include path whose .. leads here) */
#include "morsecode.h"
