!  mean_forcing_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference module mw_forcing_statistic, compiled by tests/golden/make_mean_forcing.py
!  against the module files and objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).
!  It fills SetupDT / MeshDT / Input_DataDT from flat arrays the way tests/golden/interception_driver.f90 does, calls the
!  reference's compute_mean_forcing (smash/solver/routine/mw_forcing_statistic.f90:18-75) and hands mean_prcp / mean_pet back.
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module mean_forcing_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mw_sparse_storage
    use mw_forcing_statistic, only: compute_mean_forcing

    implicit none

contains

    !  icfg = (nrow; ncol; nt; ng; sparse_storage 0/1; nrep)
    !  arrays column-major as the reference holds them, path and gauge_pos 1-based
    !  elapsed: seconds of the fastest of nrep calls of the routine alone (the set-up is not timed)
    subroutine mf_run(icfg, flwdir, path, active_cell, gauge_pos, prcp, pet, mean_prcp, mean_pet, elapsed) bind(C, name="mf_run")

        integer(c_int), intent(in) :: icfg(6)
        integer(c_int), intent(in) :: flwdir(icfg(1), icfg(2)), path(2, icfg(1)*icfg(2)), active_cell(icfg(1), icfg(2))
        integer(c_int), intent(in) :: gauge_pos(icfg(4), 2)
        real(c_float), intent(in) :: prcp(icfg(1), icfg(2), icfg(3)), pet(icfg(1), icfg(2), icfg(3))
        real(c_float), intent(inout) :: mean_prcp(icfg(4), icfg(3)), mean_pet(icfg(4), icfg(3))
        real(c_double), intent(inout) :: elapsed

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        integer :: nrow, ncol, nt, ng, t, rep
        integer(8) :: c0, c1, crate
        real(c_double) :: one

        nrow = icfg(1); ncol = icfg(2); nt = icfg(3); ng = icfg(4)
        setup%structure = "gr-b"
        setup%sparse_storage = (icfg(5) .ne. 0)
        setup%ntime_step = nt
        setup%mean_forcing = .true.
        call SetupDT_initialise(setup, 0, ng)

        call MeshDT_initialise(mesh, setup, nrow, ncol, ng)
        mesh%flwdir = flwdir
        mesh%path = path
        mesh%active_cell = active_cell
        mesh%gauge_pos = gauge_pos
        mesh%nac = count(active_cell .eq. 1)
        if (setup%sparse_storage) call compute_rowcol_to_ind_sparse(mesh)

        call Input_DataDT_initialise(input_data, setup, mesh)
        if (setup%sparse_storage) then
            do t = 1, nt
                call sparse_matrix_to_vector_r(mesh, prcp(:, :, t), input_data%sparse_prcp(:, t))
                call sparse_matrix_to_vector_r(mesh, pet(:, :, t), input_data%sparse_pet(:, t))
            end do
        else
            input_data%prcp = prcp
            input_data%pet = pet
        end if

        elapsed = huge(1._c_double)
        do rep = 1, max(1, icfg(6))
            call system_clock(c0, crate)
            call compute_mean_forcing(setup, mesh, input_data)
            call system_clock(c1)
            one = real(c1 - c0, c_double)/real(crate, c_double)
            if (one .lt. elapsed) elapsed = one
        end do
        mean_prcp = input_data%mean_prcp
        mean_pet = input_data%mean_pet

    end subroutine mf_run

end module mean_forcing_driver
