// processor/audio-filter.hpp — a node the reference has no class for: a linear-phase FIR filter (low-pass, high-pass, band-pass, band-stop)
// on the library's FFT fast convolution (nae_fir_*; DESIGN.md §3, "K9 FIR filter").  Registered by infra::register_extension_processors().
// Its process_payload stands in audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_filter": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "kind"      "lowpass" | "highpass" | "bandpass" | "bandstop"                    (default "lowpass")
	//   "f_lo"      Hz: the high-pass corner, the lower edge of a band                  (default 100)
	//   "f_hi"      Hz: the low-pass corner, the upper edge of a band                   (default 1000)
	//   "taps"      odd, 1 ... 2049: the length L of the Kaiser-8 design (nae_fir_design) (default 513)
	//   "fft_size"  512 / 1024 / 2048 / 4096 with taps <= fft_size / 2 + 1; absent: the library's pick (nae_fir_pick_n_fft)
	// A value of the wrong type or outside these sets: Runtime_error "Wrong field: <key>".  Defaults are not written back; "fft_size" only when
	// it was given.  The taps are designed from the stream's sample rate when the first frame arrives (a corner at or above half of it is a
	// Runtime_error then).  The node compensates the filter's group delay: it drops the first (L - 1) / 2 filtered frames and flushes at the
	// end of the stream, so it delivers exactly the frames it received — output sample n is y[n + (L - 1) / 2] — as packed float frames of
	// the input frames' sizes, pts and time base.
	// the keys above as a plain copyable record: the node is one
	struct Filter_settings
	{
		enum class Kind { Lowpass, Highpass, Bandpass, Bandstop };
		static constexpr int default_taps = 513, max_taps = 2049;
		static constexpr float default_f_lo = 100, default_f_hi = 1000;
		Kind kind = Kind::Lowpass;
		float f_lo = default_f_lo, f_hi = default_f_hi;
		int taps = default_taps;
		int fft_size = 0;  // 0: the library's pick

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_filter : public infra::Processor, public Filter_settings
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
