// qt_scale_driver.cpp -- TEST INFRASTRUCTURE ONLY: QImage::scaledToWidth and convertToFormat behind a C interface, so that
// tests/test_qt_scale_restatement.py can hold tests/qt_scale_ref.py to the installed Qt byte for byte.  Built by that test
// (and by tests/golden/make_qt_scale.py) against the Qt that oracle/Makefile names; never linked or loaded by the product.
// Pixels cross the interface as R, G, B, A bytes (the layout of srh_view_upload); inside they are QRgb words of a
// Format_ARGB32 (has_alpha) or Format_RGB32 image, which is what QImage(file) makes of a PNG with / without alpha.
#include <QtGui/QImage>
#include <QtCore/QtGlobal>
#include <chrono>
#include <cstdint>

static QImage fromBytes(const uint8_t *rgba, int w, int h, int has_alpha) {
	QImage img(w, h, has_alpha ? QImage::Format_ARGB32 : QImage::Format_RGB32);
	for (int y = 0; y < h; ++y) {
		QRgb *line = reinterpret_cast<QRgb *>(img.scanLine(y));
		const uint8_t *p = rgba + static_cast<size_t>(y)*w*4;
		for (int x = 0; x < w; ++x, p += 4) line[x] = qRgba(p[0], p[1], p[2], has_alpha ? p[3] : 255);
	}
	return img;
}

// the raw words of a 32-bit image, whatever its format says about them (what VectorImage::fromQImage reads)
static void toBytes(const QImage &img, uint8_t *out) {
	for (int y = 0; y < img.height(); ++y) {
		const QRgb *line = reinterpret_cast<const QRgb *>(img.constScanLine(y));
		uint8_t *p = out + static_cast<size_t>(y)*img.width()*4;
		for (int x = 0; x < img.width(); ++x, p += 4) {
			p[0] = static_cast<uint8_t>(qRed(line[x])); p[1] = static_cast<uint8_t>(qGreen(line[x]));
			p[2] = static_cast<uint8_t>(qBlue(line[x])); p[3] = static_cast<uint8_t>(qAlpha(line[x]));
		}
	}
}

extern "C" {

const char *qs_qt_version() { return qVersion(); }

// scaledToWidth(dw, smooth ? Qt::SmoothTransformation : Qt::FastTransformation).  dims[0..1] = the size Qt chose (0, 0: a
// null image), dims[2] = 1 when the result is not a 32-bit image; the pixels are written when they fit cap_pixels.
int qs_scaled_to_width(const uint8_t *rgba, int w, int h, int has_alpha, int dw, int smooth, uint8_t *out, long cap_pixels, int *dims) {
	const QImage src = fromBytes(rgba, w, h, has_alpha);
	const QImage dst = src.scaledToWidth(dw, smooth ? Qt::SmoothTransformation : Qt::FastTransformation);
	dims[0] = dst.width(); dims[1] = dst.height(); dims[2] = dst.isNull() ? 0 : dst.depth() != 32;
	if (dst.isNull() || dst.depth() != 32) return 0;
	if (static_cast<long>(dst.width())*dst.height() > cap_pixels) return -1;
	toBytes(dst, out);
	return 0;
}

// Milliseconds per repetition of the two scalings of the Qt binding's ingestViewFile on an image with alpha -- smooth for the
// pixels, fast for the mask source -- without the decode and without the copies of this interface (profiles/qt_scale_timing.py)
double qs_time_ingest_ms(const uint8_t *rgba, int w, int h, int dw, int repeat) {
	const QImage src = fromBytes(rgba, w, h, 1);
	long sink = 0;
	const auto t0 = std::chrono::steady_clock::now();
	for (int r = 0; r < repeat; ++r) {
		const QImage a = src.scaledToWidth(dw, Qt::SmoothTransformation);
		const QImage b = src.scaledToWidth(a.width(), Qt::FastTransformation);
		sink += a.pixel(0, 0) + b.pixel(0, 0);
	}
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return sink == -1 ? 0.0 : ms/repeat;
}

// convertToFormat(Format_ARGB32_Premultiplied) of a Format_ARGB32 image, raw words
int qs_premultiply(const uint8_t *rgba, int w, int h, uint8_t *out) {
	toBytes(fromBytes(rgba, w, h, 1).convertToFormat(QImage::Format_ARGB32_Premultiplied), out);
	return 0;
}

}
