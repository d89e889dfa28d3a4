/* Stand-ins for the widgets the Morse modem plugin's panel code names (setupDataUi, refreshOutput, the slider slots), so that
 * plugins/MorseDigitalModem/morse.cpp compiles unmodified without Qt.  Our own text: nothing here is taken from Qt or from the
 * reference.  No driven code calls any of it (the plugin's panel pointer stays NULL); every method does nothing. */
#ifndef PEBBLE_ORACLE_GUI_STANDINS_H
#define PEBBLE_ORACLE_GUI_STANDINS_H
#include "qt_standins.h"

namespace Qt {
enum ScrollBarPolicy { ScrollBarAsNeeded, ScrollBarAlwaysOff, ScrollBarAlwaysOn };
}
struct QTextOption { enum WrapMode { NoWrap, WordWrap }; };
struct QTextCursor { enum MoveOperation { Start, End }; };

class QWidget : public QObject {
public:
    QWidget(QWidget * = nullptr) {}
    void setStyleSheet(const QString &) {}
};
class QFrame : public QWidget {};
class QPainter {};
class QEvent {};

class QTextEdit : public QWidget {
public:
    enum AutoFormattingFlag { AutoNone = 0 };
    void setAutoFormatting(int) {}
    void setAcceptRichText(bool) {}
    void setReadOnly(bool) {}
    void setUndoRedoEnabled(bool) {}
    void setWordWrapMode(int) {}
    void ensureCursorVisible() {}
    void setVerticalScrollBarPolicy(int) {}
    void clear() {}
    void insertPlainText(const QString &) {}
    void moveCursor(int) {}
};
class QLabel : public QWidget {
public:
    void setText(const QString &) {}
};
class QPushButton : public QWidget {
public:
    void setCheckable(bool) {}
    void setChecked(bool) {}
};
class QComboBox : public QWidget {
public:
    void addItem(const QString &, const QVariant & = QVariant()) {}
    void setCurrentIndex(int) {}
    QVariant itemData(int) const { return QVariant(); }
};
/* the panel's speed-range slider has two handles */
class RangeSlider : public QWidget {
public:
    void setMinimum(int) {}
    void setMaximum(int) {}
    void setValue(int) {}
    void setValue2(int) {}
};
#endif
