/* stand-in for the header uic would generate from the Morse modem's data panel: the members and methods morse.cpp names.  The driver
 * never gives the plugin a parent widget, so its panel pointer stays NULL and none of this runs.  See gui_standins.h */
#ifndef PEBBLE_ORACLE_UI_DATA_MORSE_H
#define PEBBLE_ORACLE_UI_DATA_MORSE_H
#include "gui_standins.h"
namespace Ui {
class dataMorse {
public:
    void setupUi(QWidget *) {}
    QTextEdit *dataEdit = nullptr;
    QPushButton *resetButton = nullptr;
    QPushButton *freezeButton = nullptr;
    QComboBox *outputOptionBox = nullptr;
    RangeSlider *wpmSlider = nullptr;
    QLabel *wpmLow = nullptr;
    QLabel *wpmHigh = nullptr;
    QLabel *wpmCurrent = nullptr;
};
}
#endif
