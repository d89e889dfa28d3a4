/* stand-in: see qt_standins.h */
#include "../qt_standins.h"
