// processor/audio-saturation.hpp — a node the reference has no class for: drive, saturation and clipping on the library's oversampled
// waveshaper (nae_sat_*; DESIGN.md §3, "K18 saturation").  Registered by infra::register_saturation_processors().  Its process_payload stands
// in audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_saturation": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "drive_db"    0 ... 48: the gain in front of the curve                                    (default 12)
	//   "curve"       "soft" | "hard": the Pade form of tanh, or a clipper at +-1                 (default "soft")
	//   "bias"        0 ... 1: an offset in front of the curve, taken out behind it: the curve
	//                 becomes asymmetric and makes even harmonics, the "tube" character           (default 0)
	//   "oversample"  1 | 2 | 4 | 8: the rate the curve runs at, in sample rates                  (default 4)
	//   "output_db"   -24 ... 24: the level of the shaped signal                                  (default 0)
	//   "mix"         0 ... 1: shaped against dry                                                 (default 1)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  With a bias
	// the output carries no offset while the input is silent, but a driven signal gains one: an audio_eq high-pass behind the node removes it.
	// The node drops the library's latency (32 samples at oversample 2, 4 and 8, none at 1) in front, as audio_filter drops its group
	// delay, and delivers exactly the frames it received, as packed float frames of their sizes, pts and time base.
	// the keys above as a plain copyable record: the node is one
	struct Saturation_settings
	{
		enum class Curve { Soft, Hard };
		static constexpr double default_drive_db = 12, default_bias = 0, default_output_db = 0, default_mix = 1;
		static constexpr int default_oversample = 4;
		double drive_db = default_drive_db, bias = default_bias, output_db = default_output_db, mix = default_mix;
		int oversample = default_oversample;
		Curve curve = Curve::Soft;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_saturation : public infra::Processor, public Saturation_settings
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
