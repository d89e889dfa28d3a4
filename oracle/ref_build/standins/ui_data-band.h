/* stand-in for the header uic would generate from the demodulators' data panel: Demod keeps a pointer to it and the driven classes
 * never touch it.  See qt_standins.h */
#ifndef PEBBLE_ORACLE_UI_DATA_BAND_H
#define PEBBLE_ORACLE_UI_DATA_BAND_H
namespace Ui {
class dataBand {
public:
    dataBand() {}
};
}
#endif
