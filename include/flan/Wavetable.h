// flan/Wavetable.h -- a table of single-cycle waveforms and its synthesis (mirrors the reference's src/flan/Wavetable.h).  The table is a
// flan::Audio of `wavelength` frames per waveform; it is built, played and edited on the device (flan_amd/csrc/wavetable.hip, DESIGN.md
// 4.23).  Not offered: graph_waveform_range and save_waveform_range_to_bmp (graphing is outside this library).
#pragma once
#include <vector>

#include "flan/Audio.h"
#include "flan/Function.h"
#include "flan/defines.h"

namespace flan {

class Wavetable
	{
public:
	enum class SnapMode { None, Zero, Level };
	enum class PitchMode { None, Local, Global };

	Wavetable( const Wavetable & ) = delete;
	Wavetable & operator=( const Wavetable & ) = delete;
	Wavetable( Wavetable && ) = default;
	Wavetable & operator=( Wavetable && ) = default;
	~Wavetable() = default;

	/** Cuts `source` into waveforms and resamples each to `wavelength` frames (Wavetable.cpp:134-233).  The starts are walked on the host:
	 *  pitch from source.filter_1pole_lowpass( 4000, 2 ) through get_local_wavelengths( c, 0, -1, wavelength, 128, 1, 32 ) and
	 *  get_average_wavelength( locals, .2, 64 ), snapping on the unfiltered source; a channel that falls back from Global to None leaves
	 *  None in force for the channels after it, as in the reference.  fixed < 1, a snap_ratio outside ( 0, .95 ), a null source, a
	 *  wavelength that is no power of two in 64 ... 8192 or a waveform of more than 16384 source frames give a null Wavetable. */
	Wavetable( const Audio & source, SnapMode snap_mode = SnapMode::Zero, PitchMode pitch_mode = PitchMode::Local, Frame wavelength = 2048,
		float snap_ratio = .3f, Frame fixed = 256, flan_CANCEL_ARG );
	/** num_waves waveforms sampled from f: wave k is f( k + frame / wavelength ).  (The reference writes every wave to slot 0, :247; here
	 *  wave k goes to slot k.)  Mono, 48 kHz. */
	Wavetable( const Function<Second, Amplitude> & f, int num_waves, Frame wavelength = 2048, flan_CANCEL_ARG );
	Wavetable();                                                                 // null

	/** :266-334.  `length` seconds at freq( t ) Hz, reading the table at ratio( t ) of the source's length (ratio_to_table_index), blended
	 *  between the two neighbouring waveforms when `smooth`; freq and ratio are read where a block of the resampler starts.  A null
	 *  Wavetable, a length or granularity below one frame, or a frequency the device refuses (see flanhip_wavetable_synth_plan) give a null
	 *  Audio.  The result stays device-resident until read. */
	Audio synthesize( Second length, const Function<Second, Frequency> & freq, const Function<Second, float> & ratio = 0, bool smooth = true,
		Second granularity_time = .001f, flan_CANCEL_ARG ) const;

	int get_num_waveforms( Channel channel ) const;                              // the starts of the channel, as in the reference (:359-362)
	Frame get_wavelength() const { return wavelength; }
	const Audio & get_table() const { return table; }
	bool is_null() const;

	/** The edits of :364-451, every slot once (include/flanhip.h: flanhip_wavetable_edit_dev). */
	void add_fades_in_place( Frame fade_frames = 32 );
	void remove_jumps_in_place( Frame fade_frames = 32 );
	void remove_dc_in_place();
	void normalize_in_place();

private:
	void edit( int mode, Frame fade_frames );
	Frame wavelength;
	Frame num_source_frames;
	std::vector<std::vector<Frame>> waveform_starts;
	Audio table;
	};

} // namespace flan
