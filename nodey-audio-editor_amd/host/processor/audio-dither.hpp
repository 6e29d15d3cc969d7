// processor/audio-dither.hpp — a node the reference has no class for: word-length reduction with dither and noise shaping on the library's
// dither (nae_dither_*; DESIGN.md §3, "K23 dither").  Registered by infra::register_dither_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

#include <cstdint>
#include <vector>

namespace processor
{
	// Registered as "audio_dither": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "bits"     integer 8 ... 24: the word length whose grid the output lies on                        (default 16)
	//   "dither"   "none" | "rectangular" | "triangular" | "highpass": the noise added in front of the
	//              rounding; triangular (TPDF, +-1 LSB) frees the error of the signal, highpass is
	//              triangular with a blue spectrum                                                        (default "triangular")
	//   "shaping"  "none" | "first" | "second" | "lipshitz": the error feedback's taps; lipshitz is the
	//              5-tap psychoacoustic curve designed for 44.1 kHz (it moves with the sample rate)       (default "none")
	//   "taps"     array of 1 ... 12 numbers c_1 ... c_K of NTF(z) = 1 - sum c_k z^-k, finite, their
	//              absolute sum at most 64; overrides "shaping"                                           (default absent)
	//   "seed"     integer 0 ... 2^53 - 1; channel c of the stream draws from the key of channel c        (default 1)
	// A value of the wrong type, outside these ranges or of a wrong array length: Runtime_error "Wrong field: <key>".  Defaults are not
	// written back.  The node needs no sample rate and holds nothing back: it delivers exactly the frames it received, as packed float
	// frames of their sizes, pts and time base.  It belongs last in a chain, behind audio_limiter / audio_loudness, with nothing but a format
	// conversion after it.
	// the keys above as a plain copyable record: the node is one
	struct Dither_settings
	{
		enum class Dither { Triangular, None, Rectangular, Highpass };   // the default first (node-fields.hpp, Choice)
		enum class Shaping { None, First, Second, Lipshitz };
		static constexpr int default_bits = 16;
		static constexpr uint64_t default_seed = 1;
		int bits = default_bits;
		Dither dither = Dither::Triangular;
		Shaping shaping = Shaping::None;
		std::vector<double> taps;   // empty: absent
		uint64_t seed = default_seed;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_dither : public infra::Processor, public Dither_settings
	{
	  public:

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;
		void deserialize(const Json::Value& value) override;
	};
}
