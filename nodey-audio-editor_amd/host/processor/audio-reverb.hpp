// processor/audio-reverb.hpp — a node the reference has no class for: a convolution reverb on the library's long convolution (nae_conv_*;
// DESIGN.md §3, "K10 long convolution").  Registered by infra::register_effect_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_reverb": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "rt60"         seconds, 0.1 ... 5: the decay time to -60 dB                          (default 1.5)
	//   "predelay_ms"  0 ... 200: silence in front of the tail                               (default 20)
	//   "wet"          0 ... 1: the level of the tail, whose response has unit energy        (default 0.3)
	//   "dry"          0 ... 1: the level of the direct signal                               (default 1)
	//   "seed"         integer >= 0: channel c's noise comes from seed + c                   (default 1)
	//   "fft_size"     512 / 1024 / 2048 / 4096; absent: the library's pick (nae_conv_pick_n_fft)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back; "fft_size" only
	// when it was given.  The responses — one per channel, so a stereo tail is decorrelated — are designed from the stream's sample rate when
	// the first frame arrives (nae_conv_design_reverb); one longer than the library's limits is a Runtime_error then.  The node is causal and
	// uncompensated: it delivers exactly the frames it received, as packed float frames of their sizes, pts and time base, and drops the tail
	// past the end of the stream.
	// the keys above as a plain copyable record: the node is one
	struct Reverb_settings
	{
		static constexpr double default_rt60 = 1.5, default_predelay_ms = 20, default_wet = 0.3, default_dry = 1;
		double rt60 = default_rt60, predelay_ms = default_predelay_ms, wet = default_wet, dry = default_dry;
		static constexpr uint64_t default_seed = 1;
		uint64_t seed = default_seed;
		int fft_size = 0;  // 0: the library's pick

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_reverb : public infra::Processor, public Reverb_settings
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
