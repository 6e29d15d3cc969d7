// processor/audio-eq.hpp — a node the reference has no class for: a parametric equalizer on the library's biquad cascade (nae_eq_*;
// DESIGN.md §3, "K11 biquad cascade").  Registered by infra::register_equalizer_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_eq": one audio input pin, one audio output pin.  JSON: "bands", an array of 1 ... 16 objects with the keys, all
	// optional:
	//   "kind"     "peak" | "lowshelf" | "highshelf" | "lowpass" | "highpass" | "notch"   (default "peak")
	//   "freq"     Hz, above 0: the centre or corner frequency                           (default 1000)
	//   "gain_db"  -24 ... 24; ignored by lowpass, highpass and notch                    (default 0)
	//   "q"        0.1 ... 40                                                            (default 0.707)
	// An absent or empty "bands" is a wire: the frames pass as they are.  "bands" of another type or with more than 16 entries, or an entry
	// that is no object: Runtime_error "Wrong field: bands"; a band's value of the wrong type or outside these ranges: "Wrong field: <key>".
	// Defaults are not written back.  The sections are designed from the stream's sample rate when the first frame arrives (nae_eq_design); a
	// band at or above Nyquist for that rate is a Runtime_error then.  The node delivers exactly the frames it received, as packed float
	// frames of their sizes, pts and time base, and flushes at the end of the stream.
	class Audio_eq : public infra::Processor
	{
	  public:

		enum class Kind { Peak = 0, Lowshelf, Highshelf, Lowpass, Highpass, Notch };   // NAE_EQ_PEAK ... NAE_EQ_NOTCH
		struct Band
		{
			static constexpr double default_freq = 1000, default_gain_db = 0, default_q = 0.707;
			Kind kind = Kind::Peak;
			double freq = default_freq, gain_db = default_gain_db, q = default_q;

			void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
		};
		static constexpr size_t max_bands = 16;
		std::vector<Band> bands;

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
